"""mev_sample_plans (include/marlenv.h): mev_evaluate_plans / mev_evaluate_leaves whose candidates draw
their own actions.  Two contracts are checked bit for bit: actions_out against the numpy restatement
of the stated formula (plan_noise_ref), every element of it, and every other output against
mev_evaluate_plans / mev_evaluate_leaves on the same handle fed actions_out and the groups' roots
repeated per candidate -- calls that their own tests check against the oracle.

The shared scene is test_evaluate_plans_gpu's scenario 1 (the drifting history with envs reset by
hand, so the roots' step counters are 25, 17, 17 and 10) with max_steps = 20: the candidates of env 0
are past the limit and stop at their first sub-step, those of env 3 are truncated at the third, those
of env 5 run all T = 5 rows."""
import numpy as np
import pytest

import golden_replay as G
import plan_noise_ref as PN
import test_evaluate_plans_gpu as EP
import window_ref as RR
from window_ref import DT

pytestmark = pytest.mark.gpu

ALL = EP.ALL
SEQ = EP.SEQ
E, RAYS, T, K = 6, 16, 5, 5
ROOTS = np.array([0, 3, 3, 5], np.int32)
GROUPS = len(ROOTS)
C = GROUPS * K
CFG = dict(use_team=True, max_steps=20)
LO, HI = (-0.8, -0.6), (0.7, 0.9)
SEED, COUNTER, GAMMA = 0x5EED0123456789AB, (3 << 32) | 11, 0.97
DTS = np.array([DT, DT / 2, 1.5 * DT, DT, DT], np.float32)


def draw_dist(N, seed=50, groups=GROUPS, t=T):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-0.5, 0.5, (t, groups, N, 2)).astype(np.float32)
    mean[..., 0] += np.float32(0.4)
    sigma = rng.uniform(0.2, 0.6, (t, groups, N, 2)).astype(np.float32)
    return mean, sigma


def make_handle(mev, N, dims=False):
    h, _ = EP._handle(mev, E, N, RAYS, **CFG)
    if dims:
        drng = np.random.default_rng(40)
        h.set_car_dims(np.stack([drng.uniform(40, 70, (E, N)), drng.uniform(18, 30, (E, N))], -1).astype(np.float32), None)
    EP._device_history_plain(h, EP.PLAIN["seed"])
    return h


def sample(h, mean, sigma, roots=ROOTS, leaf=True, **kw):
    args = dict(dt=DTS, gamma=GAMMA, lo=LO, hi=HI, seed=SEED, counter=COUNTER, leaf_obs=leaf)
    args.update(kw)
    return h.sample_plans(mean, sigma, roots, K, **args)


def assert_equals_evaluate(tag, h, out, roots, dts=DTS, gamma=GAMMA, leaf=True, spawn_route=None):
    ref = h.evaluate_plans(out["actions_out"], np.repeat(roots, K).astype(np.int32), dts, gamma, spawn_route=spawn_route,
                           leaf_obs=leaf)
    for k in ALL + (("leaf_obs",) if leaf else ()):
        assert G.bits_equal(out[k], ref[k]), f"{tag}: {k}"
    return ref


@pytest.fixture(scope="module", params=[2, 12])
def scene(mev, request):
    """The handle after its history, the distribution and the host-mode result (computed once, never changed)."""
    N = request.param
    h = make_handle(mev, N)
    before = EP._snap_all(h)
    mean, sigma = draw_dist(N)
    out = sample(h, mean, sigma)
    after = EP._snap_all(h)
    yield dict(h=h, N=N, mean=mean, sigma=sigma, out=out, before=before, after=after)
    h.close()


def test_actions_out_is_the_stated_formula(scene):
    S = scene
    out = S["out"]
    want = PN.sampled_actions(S["mean"], S["sigma"], K, LO, HI, SEED, COUNTER)
    assert out["actions_out"].shape == (T, C, S["N"], 2)
    assert G.bits_equal(out["actions_out"], want)  # (every row: also those after an early stop)
    a = out["actions_out"]
    for k in range(2):
        assert (a[..., k] == np.float32(LO[k])).any() and (a[..., k] == np.float32(HI[k])).any(), k
        inside = (a[..., k] > np.float32(LO[k])) & (a[..., k] < np.float32(HI[k]))
        assert inside.mean() > 0.5
    sub = out["substeps"]
    print("substeps", sub.tolist())
    assert list(S["before"]["state"]["step_count"][ROOTS]) == [25, 17, 17, 10]
    assert (sub < T).any() and (sub == T).any()
    inside = (sub > 1) & (sub < T)
    assert (inside & (out["truncated"] != 0)).any()  # (env 3: a truncation inside the window)


def test_outputs_equal_evaluate_plans(scene):
    S = scene
    assert_equals_evaluate("with leaf_obs", S["h"], S["out"], ROOTS)
    plain = sample(S["h"], S["mean"], S["sigma"], leaf=False)
    assert "leaf_obs" not in plain
    assert_equals_evaluate("without leaf_obs", S["h"], plain, ROOTS, leaf=False)
    assert G.bits_equal(plain["actions_out"], S["out"]["actions_out"])
    EP._assert_same("evaluation calls", S["before"], EP._snap_all(S["h"]))


def test_car_sizes(mev):
    N = 3
    h = make_handle(mev, N, dims=True)
    assert h.car_dims_active()
    mean, sigma = draw_dist(N)
    out = sample(h, mean, sigma)
    assert G.bits_equal(out["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, COUNTER))
    assert_equals_evaluate("per-car sizes", h, out, ROOTS)
    h.close()


def test_handle_untouched(mev, scene):
    S = scene
    EP._assert_same("sample_plans", S["before"], S["after"])
    if S["N"] != 2:
        return
    h = make_handle(mev, 2)  # (a copy: the shared scene's handle stays where the other tests expect it)
    out = sample(h, S["mean"], S["sigma"])
    for k in ALL + ("leaf_obs", "actions_out"):
        assert G.bits_equal(out[k], S["out"][k]), k
    EP._twin_step("sample_plans", mev, h, lambda: make_handle(mev, 2), 2)
    h.close()


@pytest.mark.parametrize("max_npcs", [32, 64])
def test_traffic(mev, max_npcs):
    """One ego in dense traffic: with spawn_route, and with the Philox spawner keyed by the candidate."""
    En, N, Tn, Gn = 8, 1, 4, 5
    h, ids = EP._handle(mev, En, N, RAYS, max_npcs=max_npcs, traffic=True, density=20.0, max_steps=2000)
    EP._device_history_traffic(h, EP.TRAFFIC["seed"])
    before = EP._snap_all(h)
    assert before["state"]["npc_count"].max() >= 3
    rng = np.random.default_rng(51)
    roots = rng.integers(0, En, Gn).astype(np.int32)
    mean, sigma = draw_dist(N, seed=52, groups=Gn, t=Tn)
    dts = DTS[:Tn]
    sp = rng.integers(-1, 12, (Tn, Gn * K))
    for tag, route in (("spawn_route", sp), ("philox spawner", None)):
        out = sample(h, mean, sigma, roots=roots, dt=dts, spawn_route=route)
        assert G.bits_equal(out["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, COUNTER))
        assert_equals_evaluate(tag, h, out, roots, dts=dts, spawn_route=route)
    EP._assert_same("traffic", before, EP._snap_all(h))
    h.close()


def test_traffic_without_leaf_obs(mev):
    """The smallest scene with the NPC phase and no leaf_obs (the one mode test_traffic leaves out): 2
    envs of 2 agents, 8 rays, 4 NPC slots, one group of K = 5 candidates over 3 rows, Philox spawner."""
    En, N, Tn = 2, 2, 3
    h, _ = EP._handle(mev, En, N, 8, max_npcs=4, traffic=True, density=20.0, max_steps=2000)
    EP._device_history_traffic(h, EP.TRAFFIC["seed"])
    before = EP._snap_all(h)
    assert before["state"]["npc_count"].max() >= 1
    roots = np.array([1], np.int32)
    mean, sigma = draw_dist(N, seed=53, groups=1, t=Tn)
    out = sample(h, mean, sigma, roots=roots, dt=DTS[:Tn], leaf=False)
    assert "leaf_obs" not in out
    assert G.bits_equal(out["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, COUNTER))
    assert_equals_evaluate("traffic, no leaf_obs", h, out, roots, dts=DTS[:Tn], leaf=False)
    EP._assert_same("traffic, no leaf_obs", before, EP._snap_all(h))
    h.close()


def test_chunks_cut_through_groups(mev, scene, monkeypatch):
    """MEV_LEAF_CHUNK=3 at creation, K = 5: 20 candidates in chunks of 3, every output the same."""
    S = scene
    if S["N"] != 2:
        return
    monkeypatch.setenv("MEV_LEAF_CHUNK", "3")
    h = make_handle(mev, 2)
    monkeypatch.delenv("MEV_LEAF_CHUNK")
    out = sample(h, S["mean"], S["sigma"])
    for k in ALL + ("leaf_obs", "actions_out"):
        assert G.bits_equal(out[k], S["out"][k]), k
    h.close()


def test_mean_first_sigma_zero_and_the_counter(scene):
    S = scene
    h, mean, sigma, base = S["h"], S["mean"], S["sigma"], S["out"]
    out = sample(h, mean, sigma, mean_first=True)
    a = out["actions_out"]
    clamped = np.minimum(np.maximum(mean + np.float32(0.0) * sigma, np.float32(LO)), np.float32(HI)).astype(np.float32)
    assert G.bits_equal(a[:, ::K], clamped)
    assert G.bits_equal(a, PN.sampled_actions(mean, sigma, K, LO, HI, SEED, COUNTER, mean_first=True))
    others = np.arange(C) % K != 0
    for k in ALL + ("leaf_obs",):
        x, y = (out[k], base[k])
        assert G.bits_equal(x[:, others], y[:, others]) if k in SEQ else G.bits_equal(x[others], y[others]), k
    assert G.bits_equal(a[:, others], base["actions_out"][:, others])
    assert_equals_evaluate("mean first", h, out, ROOTS)
    # sigma = 0: every candidate of a group runs the same rows
    out = sample(h, mean, np.zeros_like(sigma), leaf=False)
    a = out["actions_out"].reshape(T, GROUPS, K, S["N"], 2)
    assert all(G.bits_equal(a[:, :, j], a[:, :, 0]) for j in range(K))
    # another counter: other actions; the same counter: the same
    out = sample(h, mean, sigma, counter=COUNTER + 1, leaf=False)
    assert not G.bits_equal(out["actions_out"], base["actions_out"])
    assert G.bits_equal(out["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, COUNTER + 1))
    out = sample(h, mean, sigma, leaf=False)
    assert G.bits_equal(out["actions_out"], base["actions_out"])


def test_device_pointers(scene):
    import torch
    torch.cuda.set_device(0)
    S = scene
    h, N, base = S["h"], S["N"], S["out"]
    dev = "cuda:0"
    D = base["leaf_obs"].shape[-1]

    def garbage():
        shapes = dict(returns=((C, N), torch.float32), reward_seq=((T, C, N), torch.float32),
                      done_seq=((T, C, N), torch.uint8), status_seq=((T, C, N), torch.uint8),
                      substeps=((C,), torch.int32), terminated=((C,), torch.uint8), truncated=((C,), torch.uint8),
                      leaf_obs=((C, N, D), torch.float32), actions_out=((T, C, N, 2), torch.float32))
        return {k: torch.full(s, 77, dtype=d, device=dev) for k, (s, d) in shapes.items()}

    tm, ts = torch.as_tensor(S["mean"]).to(dev), torch.as_tensor(S["sigma"]).to(dev)
    keys = ALL + ("leaf_obs", "actions_out")
    o = garbage()
    sample(h, tm, ts, roots=torch.as_tensor(ROOTS).to(dev), out=o, device=True)
    h.sync()
    for k in keys:
        assert G.bits_equal(o[k].cpu().numpy(), base[k]), k
    # a root outside [0, E): exactly its group's K candidates are all zero, their action rows still the formula's
    bad = ROOTS.copy()
    bad[2] = E
    o = garbage()
    sample(h, tm, ts, roots=torch.as_tensor(bad).to(dev), out=o, device=True)
    h.sync()
    gone = slice(2 * K, 3 * K)
    for k in keys:
        got, want = o[k].cpu().numpy(), base[k].copy()
        if k in SEQ:
            want[:, gone] = 0
        elif k != "actions_out":
            want[gone] = 0
        assert G.bits_equal(got, want), k
    # only `returns`: nothing else is written
    o = garbage()
    sample(h, tm, ts, roots=torch.as_tensor(ROOTS).to(dev), out=dict(returns=o["returns"]), device=True, leaf=False)
    h.sync()
    assert G.bits_equal(o["returns"].cpu().numpy(), base["returns"])
    for k in keys:
        if k != "returns":
            assert (o[k] == 77).all(), k
    EP._assert_same("device calls", S["before"], EP._snap_all(h))


def test_errors(mev):
    import ctypes
    N = 1
    h, _ = EP._handle(mev, 2, N, RAYS, use_team=False, max_steps=0)
    EP._device_history_plain(h, 35, steps=5, reset_at={})
    before = EP._snap_all(h)
    mean, sigma = draw_dist(N, groups=2, t=3)
    ok = dict(dt=DT, lo=LO, hi=HI, seed=1, counter=2)
    roots = np.array([0, 1], np.int32)
    h.sample_plans(mean, sigma, roots, 2, **ok)
    bad = [dict(lo=(0.8, -1.0)), dict(hi=(1.0, -0.7)), dict(lo=(-np.inf, -1.0)), dict(hi=(np.nan, 1.0)),
           dict(sample_flags=2), dict(flags=mev._capi.MEV_AUTO_RESET), dict(out=dict(returns=None))]
    for kw in bad:
        with pytest.raises(mev.MevError):
            h.sample_plans(mean, sigma, roots, 2, **dict(ok, **kw))
    with pytest.raises(mev.MevError):  # samples = 0: no candidates
        h.sample_plans(mean, sigma, roots, 0, **ok)
    with pytest.raises(mev.MevError):  # more rows than MEV_MAX_REPEAT
        m = np.zeros((mev._capi.MEV_MAX_REPEAT + 1, 2, N, 2), np.float32)
        h.sample_plans(m, m, roots, 2, **ok)
    with pytest.raises(mev._capi.IndexRangeError):
        h.sample_plans(mean, sigma, [0, 2], 2, **ok)
    with pytest.raises(mev._capi.IndexRangeError):
        h.sample_plans(mean, sigma, [-1, 0], 2, **ok)
    # straight through the C ABI: actions given, mean or sigma missing, candidates != groups * samples
    lib, cap = mev.load_library(), mev._capi
    ret = np.zeros((4, N), np.float32)

    def call(**kw):
        sa = cap.MevSampleArgs()
        sa.eval.roots, sa.eval.candidates, sa.eval.length, sa.eval.dt = cap._ptr(roots), 4, 3, DT
        sa.eval.returns = cap._ptr(ret)
        sa.mean, sa.sigma, sa.groups, sa.samples = cap._ptr(mean), cap._ptr(sigma), 2, 2
        sa.lo, sa.hi = (ctypes.c_float * 2)(*LO), (ctypes.c_float * 2)(*HI)
        for k, v in kw.items():
            setattr(sa.eval if k in ("actions", "candidates") else sa, k, v)
        return lib.mev_sample_plans(h._h, ctypes.byref(sa))

    assert call() == 0
    assert call(actions=cap._ptr(np.zeros((3, 4, N, 2), np.float32))) == -1
    assert call(mean=None) == -1 and call(sigma=None) == -1
    assert call(candidates=5) == -1 and call(groups=0) == -1 and call(samples=3) == -1
    # host-mode shape mismatches are ValueErrors
    with pytest.raises(ValueError):
        h.sample_plans(mean, sigma[:, :1], roots, 2, **ok)
    with pytest.raises(ValueError):
        h.sample_plans(mean, sigma, [0, 1, 1], 2, **ok)
    EP._assert_same("refused calls", before, EP._snap_all(h))
    h.close()


def _vec_layer(mev, backend):
    import pkgload
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    En, N, Tn, Gn = 4, 2, 3, 3
    v = vec_env.VecIntersectionEnv(En, N, lidar_rays=RAYS, use_team_reward=True, max_steps=10, backend=backend)
    RR.set_routes(v.handle)
    rng = np.random.default_rng(9)
    for t in range(4):
        v.step(RR.draw(rng, En, N, 0.6)[0])
    state = {k: x.copy() for k, x in v.handle.get_state().items()}
    roots = np.array([2, 0, 2], np.int32)
    mean, sigma = draw_dist(N, groups=Gn, t=Tn)
    out = v.sample_plans(mean, sigma, roots, K, dt=DT, gamma=0.9, lo=LO, hi=HI, seed=SEED, counter=5, leaf_obs=True,
                         copy=True)
    assert set(out) == set(ALL) | {"leaf_obs", "actions_out"}
    ref = v.evaluate_plans(out["actions_out"], np.repeat(roots, K).astype(np.int32), dt=DT, gamma=0.9, leaf_obs=True, copy=True)
    new = v.update_plans(out["actions_out"], K, returns=out["returns"], mode="elites", elites=2, sigma_min=0.05)
    if backend == "torch":
        out, ref, new = ({k: x.cpu().numpy() for k, x in d.items()} for d in (out, ref, new))
    assert G.bits_equal(out["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, 5))
    for k in ALL + ("leaf_obs",):
        assert G.bits_equal(out[k], ref[k]), k
    want = PN.elites(out["actions_out"], PN.scores_of(out["returns"]), K, 2, 0.05)
    assert set(new) == set(want)
    for k in want:
        assert G.bits_equal(new[k], want[k]), k
    after = v.handle.get_state()
    for k in state:
        assert G.bits_equal(state[k], after[k]), k
    v.close()


def test_vec_env_numpy(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch(mev):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the device")
    _vec_layer(mev, "torch")
