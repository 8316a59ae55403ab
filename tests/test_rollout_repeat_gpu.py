"""mev_rollout_policy_repeat (include/marlenv.h): T decisions of observe -> MLP policy -> frame-skip step in one
launch, checked bit for bit against the loop it is defined as.  Handle A runs the call; handle B, with the same
config, seed and history, runs rollout_repeat_ref.rollout_repeat_ref -- the numpy policy (pinned to libm's fmaf by
test_policy_ref.py) around the unchanged Handle.step_repeat, which the existing suite pins to the oracle.  Compared:
every element of every *_seq array and of substeps_seq, the last outputs, the whole state, the car sizes, the
diagnostics, the snapshot bytes, and the outputs of one further plain step on both handles (with traffic that
step's Philox spawner shows that the counter advanced by T * n).

The conditions that keep a case from passing vacuously are asserted on the reference's data alone."""
import ctypes

import numpy as np
import pytest

import golden_replay as G
import plan_noise_ref as PN
import policy_ref as PR
import rollout_repeat_ref as RRR
import test_evaluate_plans_gpu as EP
import test_rollout_policy_gpu as RP
import test_rollout_values_gpu as RV
import window_ref as RR
from rollout_repeat_ref import ALL, ALL_VALUES, SEQS
from window_ref import DT, OUT_KEYS

pytestmark = pytest.mark.gpu

MEV_E_INVALID = -1  # include/marlenv.h


def make(mev, E, N, rays, history=0, one_car=False, **cfg):
    """RP.make; one_car: car 0 of env 0 is 55 x 24 px before the history (per-car sizes: the runtime row)."""
    if not one_car:
        return RP.make(mev, E, N, rays, history=history, **cfg)
    h = RP.make(mev, E, N, rays, history=0, **cfg)
    ego = np.tile(np.array([54.0, 24.0], np.float32), (E, N, 1))
    ego[0, 0, 0] = 55.0
    h.set_car_dims(ego, None)
    rng = np.random.default_rng(5)
    for _ in range(history):
        a, _ = RR.draw(rng, E, N, 0.6, 1, False)
        h.step(a, DT)
    return h


def one_more_step(tag, hs):
    """One plain step (auto-reset, the Philox spawner) on every handle: the same outputs, the same handles."""
    a, _ = RR.draw(np.random.default_rng(77), hs[0].E, hs[0].N, 0.5)
    outs = [h.step(a, DT, auto_reset=True) for h in hs]
    for o in outs[1:]:
        for k in OUT_KEYS:
            assert G.bits_equal(outs[0][k], o[k]), f"{tag}: the step after the call: {k}"
    for h in hs[1:]:
        RP.same_handles(tag + ": after one more step", hs[0], h)


def last_outputs(tag, h, ref):
    for k, v in h.get_outputs().items():
        assert G.bits_equal(v, RP.B_last(ref, k, v)), f"{tag}: last output {k}"


# ---- 1: every k_rollout row, n = 2 and 3, T = 1 and 4, two policies, with and without value_seq ----

SHAPES = dict(RV.SHAPES)
SHAPES["traffic 32 slots 4x1x16 spawn_route"] = (dict(RV.SHAPES["traffic 32 slots 4x1x16"][0], replay=True), 1)
SHAPES["runtime row 3x8x64, one car 55x24"] = (dict(E=3, N=8, rays=64, history=6, max_steps=2000, one_car=True), 0)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hidden", [(64, 64), (5, 3)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_row(mev, shape, hidden, n, T):
    cfg, row = SHAPES[shape]
    cfg = dict(cfg)
    E, N, rays, replay = cfg.pop("E"), cfg.pop("N"), cfg.pop("rays"), cfg.pop("replay", False)
    mk = lambda: make(mev, E, N, rays, **cfg)
    A, Av, B = mk(), mk(), mk()
    tag = f"{shape} {hidden} n={n} T={T}"
    assert A.rollout_row() == row and A.car_dims_active() == bool(cfg.get("one_car")), tag
    W, Bs = RP.net(A.D, hidden, 30 + len(hidden) + hidden[0])
    wv, bv = RV.head(hidden[-1], 41)
    route = np.random.default_rng(31).integers(-1, 12, (T, n, E)) if replay else None
    kw = dict(dt=DT, auto_reset=bool(cfg.get("traffic")), spawn_route=route)
    ref = RRR.rollout_repeat_ref(B, W, Bs, T, n, wv=wv, bv=bv, **kw)
    out = A.rollout_policy(A.policy(W, Bs), T, repeat=n, outputs=ALL, **kw)
    pv = Av.policy(W, Bs)
    pv.set_value_head(wv, bv)
    outv = Av.rollout_policy(pv, T, repeat=n, outputs=ALL_VALUES, **kw)
    assert set(out) == set(ALL) and set(outv) == set(ALL_VALUES)
    RRR.assert_all(tag, out, ref, ALL)
    RRR.assert_all(tag + " with value_seq", outv, ref, ALL_VALUES)
    for name, h in (("", A), (" with value_seq", Av)):
        RP.same_handles(tag + name, h, B)  # get_state, get_outputs, get_car_dims, diagnostics, snapshot bytes
        last_outputs(tag + name, h, ref)
    RP.conditions(tag, ref, T)
    assert (ref["substeps_seq"] >= 1).all() and (ref["substeps_seq"] == n).any(), tag
    v = ref["value_seq"]
    assert np.isfinite(v).all() and len(np.unique(v)) > 1, tag + ": the values do not vary"
    if cfg.get("traffic") and T > 1:
        assert (ref["npc_count"] >= 1).any(), tag
    one_more_step(tag, (A, Av, B))
    for h in (A, Av, B):
        h.close()


# ---- 2: repeat = 1 is mev_rollout_policy and mev_rollout_policy_values ----

@pytest.mark.parametrize("shape", ["fixed row 3x8x64", "traffic 32 slots 4x1x16"])
def test_repeat_one_is_the_plain_call(mev, shape):
    cfg, _ = SHAPES[shape]
    cfg = dict(cfg)
    E, N, rays, T = cfg.pop("E"), cfg.pop("N"), cfg.pop("rays"), 5
    hs = [make(mev, E, N, rays, **cfg) for _ in range(4)]  # the call, the call with values, the two plain calls
    snaps = [h.snapshot() for h in hs]
    assert all(G.bits_equal(snaps[0], s) for s in snaps[1:])  # the same snapshot
    W, Bs = RP.net(hs[0].D, (16, 16), 61)
    wv, bv = RV.head(16, 62)
    pols = [h.policy(W, Bs) for h in hs]
    pols[1].set_value_head(wv, bv)
    pols[3].set_value_head(wv, bv)
    kw = dict(dt=DT, auto_reset=bool(cfg.get("traffic")), sigma=(0.2, 0.1), seed=5, counter=9)
    rep = hs[0].rollout_policy(pols[0], T, repeat=1, outputs=ALL, **kw)  # (substeps_seq: the new entry point)
    repv = hs[1].rollout_policy(pols[1], T, repeat=1, outputs=ALL_VALUES, **kw)
    plain = hs[2].rollout_policy(pols[2], T, **kw)
    values = hs[3].rollout_policy(pols[3], T, outputs=SEQS + ("value_seq",), **kw)
    RRR.assert_all(shape + ": against mev_rollout_policy", rep, plain, SEQS)
    RRR.assert_all(shape + ": against mev_rollout_policy_values", repv, values, SEQS + ("value_seq",))
    assert (rep["substeps_seq"] == 1).all() and (repv["substeps_seq"] == 1).all()
    RP.same_handles(shape + ": against mev_rollout_policy", hs[0], hs[2])
    RP.same_handles(shape + ": against mev_rollout_policy_values", hs[1], hs[3])
    one_more_step(shape, hs)
    for h in hs:
        h.close()


# ---- 3: ends inside a window: max_steps = 5, n = 4, T = 5, auto-reset, respawn, noise; host and device ----

CASE3 = dict(E=3, N=8, rays=64, n=4, T=5, dt=1.0, sigma=(0.3, 0.25), seed=0x5EED0123456789AB, counter=(3 << 32) | 11,
             wseed=51, steer=0.9)


@pytest.fixture(scope="module")
def case3(mev):
    """The two references of case 3 (with and without MEV_AUTO_RESET), both forms each; computed once."""
    C = CASE3
    mk = lambda: make(mev, C["E"], C["N"], C["rays"], history=1, max_steps=5, respawn=True)
    W, Bs = RP.net(127, (16, 16), C["wseed"], steer=C["steer"])
    wv, bv = RV.head(16, 52)
    kw = dict(dt=C["dt"], sigma=C["sigma"], seed=C["seed"], counter=C["counter"])
    refs = {}
    for auto in (True, False):
        B, S = mk(), mk()
        refs[auto] = RRR.rollout_repeat_ref(B, W, Bs, C["T"], C["n"], wv=wv, bv=bv, auto_reset=auto, **kw)
        seq = RRR.rollout_repeat_ref(S, W, Bs, C["T"], C["n"], wv=wv, bv=bv, auto_reset=auto, form="sequence", **kw)
        RRR.assert_all(f"case 3 auto_reset={auto}: the step_sequence form", seq, refs[auto], ALL_VALUES)
        RP.same_handles(f"case 3 auto_reset={auto}: the step_sequence form", S, B)
        refs[auto]["sub_done"], refs[auto]["sub_status"] = seq["sub_done"], seq["sub_status"]
        refs[auto]["handle"] = B
        S.close()
    yield dict(mk=mk, W=W, Bs=Bs, wv=wv, bv=bv, kw=kw, refs=refs)
    for r in refs.values():
        r["handle"].close()


def test_case3_conditions_on_the_reference(case3):
    """(a) windows cut short and windows that run out, (b) a latched done from a non-final sub-step of its window,
    (c) a decision that begins with an auto-reset -- all from the reference's data."""
    ref, n = case3["refs"][True], CASE3["n"]
    k = ref["substeps_seq"]
    print("case 3: substeps", k.tolist(), "status counts", np.bincount(ref["status_seq"].reshape(-1), minlength=6).tolist())
    assert (k < n).any() and (k == n).any()                                                  # (a)
    last = np.arange(n)[None, :, None, None] == (k[:, None, :, None] - 1)                    # [T][n][E][1]: the stop
    early = (ref["sub_done"] != 0) & ~last & (np.arange(n)[None, :, None, None] < k[:, None, :, None])
    assert early.any()                                                                       # (b)
    t, s, e, i = np.argwhere(early)[0]
    assert ref["done_seq"][t, e, i] == 1
    later = ref["sub_done"][t, s + 1:k[t, e], e, i] != 0
    if not later.any():  # the latched status is that sub-step's, not the stop's
        assert ref["status_seq"][t, e, i] == ref["sub_status"][t, s, e, i]
    assert ref["reset_first"][1:].any()                                                      # (c)
    assert ((ref["done_seq"] != 0) & (ref["status_seq"] >= 2)).any()  # a crash or a success
    off = case3["refs"][False]
    assert (off["truncated_seq"][1:] != 0).all() and not off["reset_first"].any()  # never reset: truncated ever after


@pytest.mark.parametrize("auto", [True, False])
def test_case3_host_and_device(mev, case3, auto):
    import torch
    torch.cuda.set_device(0)
    C, S = CASE3, case3
    ref, B = S["refs"][auto], S["refs"][auto]["handle"]
    tag = f"case 3 auto_reset={auto}"
    A = S["mk"]()
    pol = A.policy(S["W"], S["Bs"])
    pol.set_value_head(S["wv"], S["bv"])
    out = A.rollout_policy(pol, C["T"], repeat=C["n"], outputs=ALL_VALUES, auto_reset=auto, **S["kw"])
    RRR.assert_all(tag, out, ref, ALL_VALUES)
    RP.same_handles(tag, A, B)
    Ad = S["mk"]()
    dw = lambda ws: [torch.as_tensor(w).cuda() for w in ws]
    pd = Ad.policy(dw(S["W"]), dw(S["Bs"]), device=True)
    pd.set_value_head(torch.as_tensor(S["wv"]).cuda(), torch.as_tensor(S["bv"]).cuda(), device=True)
    od = Ad.rollout_policy(pd, C["T"], repeat=C["n"], outputs=ALL_VALUES, device=True, auto_reset=auto, **S["kw"])
    Ad.sync()
    assert all(o.is_cuda for o in od.values()) and od["substeps_seq"].dtype == torch.int32
    RRR.assert_all(tag + ", device pointers", od, ref, ALL_VALUES)
    last_outputs(tag + ", device pointers", Ad, ref)  # (row T - 1 of the caller's arrays)
    RP.same_handles(tag + ", device pointers", Ad, B)
    A.close(), Ad.close()


# ---- 4: obs_seq NULL (the rows read in place), and each *_seq array absent in turn ----

@pytest.fixture(scope="module")
def case4(mev):
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: make(mev, E, N, rays, history=3, max_steps=4, respawn=True)
    W, Bs = RP.net(127, (16, 16), 18)
    wv, bv = RV.head(16, 54)
    B = mk()
    kw = dict(dt=DT, auto_reset=True, sigma=(0.2, 0.1), seed=4, counter=2)
    ref = RRR.rollout_repeat_ref(B, W, Bs, T, n, wv=wv, bv=bv, **kw)
    assert (ref["substeps_seq"] < n).any() and (ref["substeps_seq"] == n).any()
    yield dict(mk=mk, W=W, Bs=Bs, wv=wv, bv=bv, T=T, n=n, kw=kw, ref=ref, B=B)
    B.close()


@pytest.mark.parametrize("absent", ALL_VALUES)
def test_each_output_absent_in_turn(case4, absent):
    S = case4
    A = S["mk"]()
    pol = A.policy(S["W"], S["Bs"])
    pol.set_value_head(S["wv"], S["bv"])
    keys = tuple(k for k in ALL_VALUES if k != absent)
    out = A.rollout_policy(pol, S["T"], repeat=S["n"], outputs=keys, **S["kw"])
    assert set(out) == set(keys)
    RRR.assert_all(f"without {absent}", out, S["ref"], keys)  # (obs_seq absent: the policy read the rows in place)
    last_outputs(f"without {absent}", A, S["ref"])           # the handle's own buffers hold row T - 1
    RP.same_handles(f"without {absent}", A, S["B"])
    A.close()


# ---- 5: the noise word index is the decision, and the clamp ----

def test_noise_word_is_the_decision(mev):
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: make(mev, E, N, rays, history=3, max_steps=2000)
    A, B, Bn = mk(), mk(), mk()
    W, Bs = RP.net(A.D, (16, 16), 19)
    kw = dict(dt=DT, sigma=(0.8, 0.7), lo=(-0.5, -0.25), hi=(0.75, 0.5), seed=0xABCDEF12345, counter=(7 << 32) | 5)
    out = A.rollout_policy(A.policy(W, Bs), T, repeat=n, outputs=ALL, **kw)
    ref = RRR.rollout_repeat_ref(B, W, Bs, T, n, **kw)
    RRR.assert_all("case 5", out, ref, ALL)
    e, i = np.meshgrid(np.arange(E), np.arange(N), indexing="ij")
    for t in range(T):  # straight from plan_noise_ref at word index t
        eps = PN.noise(kw["seed"], kw["counter"], e, i, t)
        assert G.bits_equal(out["actions_seq"][t], PR.act(out["mean_seq"][t], kw["sigma"], kw["lo"], kw["hi"], eps)), t
    a = ref["actions_seq"]
    assert ((a == np.float32(-0.5)) | (a == np.float32(0.75))).any() and ((a > -0.5) & (a < 0.75)).any()  # clamped and not
    wrong = RRR.rollout_repeat_ref(Bn, W, Bs, T, n, word=lambda t: t * n, **kw)  # the sub-step's index instead
    assert G.bits_equal(wrong["actions_seq"][0], out["actions_seq"][0])
    assert not G.bits_equal(wrong["actions_seq"][1:], out["actions_seq"][1:])
    for h in (A, B, Bn):
        h.close()


# ---- 6: refused calls leave the handle untouched ----

def test_refusals(mev):
    cap, lib = mev._capi, mev.load_library()
    E, N, rays = 2, 2, 8
    h = make(mev, E, N, rays, history=3, max_steps=2000)
    other = make(mev, E, N, rays)
    W, Bs = RP.net(h.D, (16, 16), 21)
    wv, bv = RV.head(16, 57)
    pol, foreign, bare = h.policy(W, Bs), other.policy(W, Bs), h.policy(W, Bs)
    pol.set_value_head(wv, bv)
    foreign.set_value_head(wv, bv)
    ok = dict(dt=DT, outputs=ALL_VALUES, repeat=2)
    h.rollout_policy(pol, 2, **ok)
    mid = EP._snap_all(h)
    bad = [dict(repeat=0), dict(repeat=cap.MEV_MAX_REPEAT + 1), dict(T=241, repeat=17),  # T * n = 4097
           dict(policy=bare), dict(policy=None), dict(policy=foreign), dict(flags=cap.MEV_GATHER_TO_ROOT),
           dict(T=0), dict(T=cap.MEV_MAX_ROLLOUT + 1, repeat=1, outputs=("substeps_seq",)), dict(flags=0x100),
           dict(lo=(0.5, -1.0), hi=(0.4, 1.0)), dict(sigma=(np.nan, 0.1))]
    assert 241 * 17 == cap.MEV_MAX_ROLLOUT_SUBSTEPS + 1
    for kw in bad:
        args = dict(ok, policy=pol, T=2)
        args.update(kw)
        with pytest.raises(mev.MevError) as err:
            h.rollout_policy(args.pop("policy"), args.pop("T"), **args)
        assert f"error {MEV_E_INVALID}:" in str(err.value), kw
        EP._assert_same(f"refused {kw}", mid, EP._snap_all(h))
    # straight at the C boundary: the return code is MEV_E_INVALID
    ra = cap.MevRolloutRepeatArgs()
    ra.rollout.policy, ra.rollout.length, ra.rollout.dt = pol._p, 2, DT
    ra.rollout.lo = (ctypes.c_float * 2)(-1.0, -1.0)
    ra.rollout.hi = (ctypes.c_float * 2)(1.0, 1.0)
    for rep in (0, 65):
        ra.repeat = rep
        assert lib.mev_rollout_policy_repeat(h._h, ctypes.byref(ra)) == MEV_E_INVALID
    ra.rollout.length, ra.repeat = 241, 17
    assert lib.mev_rollout_policy_repeat(h._h, ctypes.byref(ra)) == MEV_E_INVALID
    assert lib.mev_rollout_policy_repeat(h._h, None) == MEV_E_INVALID
    EP._assert_same("refused calls at the C boundary", mid, EP._snap_all(h))
    # in_dim != obs_dim: a handle's obs_dim never changes and a policy is opaque, so no caller can bring such a
    # policy to the call; it is refused, with the same code, where it is made
    with pytest.raises(mev.MevError) as err:
        h.policy(*RP.net(h.D - 1, (16, 16), 1))
    assert f"error {MEV_E_INVALID}:" in str(err.value)
    EP._assert_same("refused policy", mid, EP._snap_all(h))
    # an unsupported shape: obs_dim above 31 + 128
    wide = mev.Handle(num_envs=2, num_agents=1, lidar_rays=8, obs_dim=31 + 129, device=0)
    assert wide.rollout_row() == -1
    wp = wide.policy(*RP.net(160, (8,), 1))
    sw = EP._snap_all(wide)
    with pytest.raises(mev.MevError) as err:
        wide.rollout_policy(wp, 2, dt=DT, repeat=2)
    assert f"error {MEV_E_INVALID}:" in str(err.value)
    EP._assert_same("unsupported shape", sw, EP._snap_all(wide))
    # after all that the call still runs, from where the refused ones left the handle: where it was
    twin = make(mev, E, N, rays, history=3, max_steps=2000)
    RRR.rollout_repeat_ref(twin, W, Bs, 2, 2, dt=DT, wv=wv, bv=bv)
    r = RRR.rollout_repeat_ref(twin, W, Bs, 2, 2, dt=DT, wv=wv, bv=bv)
    RRR.assert_all("after the refused calls", h.rollout_policy(pol, 2, **ok), r, ALL_VALUES)
    for x in (h, other, twin, wide):
        x.close()


# ---- 7: the vector env layer: rollout(..., repeat=3) with value_seq and substeps_seq, then gae ----

def _vec_layer(mev, backend):
    import pkgload
    import torch
    import actor_critic_ref as AC
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, T, n = 3, 8, 4, 3

    def mkv():
        v = vec_env.VecIntersectionEnv(E, N, lidar_rays=64, max_steps=7, backend=backend)
        RR.set_routes(v.handle)
        return v

    v, twin = mkv(), mkv()
    assert v.handle.rollout_row() == RP.ROW_FIXED
    torch.manual_seed(3)
    nn = torch.nn
    mod = nn.Sequential(nn.Linear(v.obs_dim, 16), nn.ReLU(), nn.Linear(16, 16), nn.ReLU(), nn.Linear(16, 2))
    critic = nn.Linear(16, 1)
    with torch.no_grad():
        mod[4].bias.copy_(torch.tensor([0.6, 0.0]))
    if backend == "torch":
        mod, critic = mod.cuda(), critic.cuda()
    host = lambda x: x.detach().cpu().numpy().copy()
    W, Bs = [host(mod[i].weight) for i in (0, 2, 4)], [host(mod[i].bias) for i in (0, 2, 4)]
    wv, bv = host(critic.weight), host(critic.bias)
    pol = v.make_policy(mod, value=critic)
    outputs = mev._capi.ROLLOUT_OUTPUTS + ("value_seq", "substeps_seq")
    out = v.rollout(pol, T, sigma=(0.2, 0.1), seed=9, counter=1, outputs=outputs, repeat=n, copy=True)
    assert set(out) == set(outputs) | {"ended_before"}
    if backend == "torch":
        assert all(x.is_cuda for x in out.values())
    ref = RRR.rollout_repeat_ref(twin.handle, W, Bs, T, n, sigma=(0.2, 0.1), seed=9, counter=1, auto_reset=True,
                                 wv=wv, bv=bv)
    RRR.assert_all(f"vec env {backend}", out, ref, ALL_VALUES + ("ended_before",))
    assert (ref["truncated_seq"][:-1] != 0).any() and (ref["substeps_seq"] < n).any()
    g = v.gae(out, 0.99, 0.95)
    adv, ret, valid = AC.gae_ref(ref["reward_seq"], ref["value_seq"], ref["done_seq"], ref["terminated_seq"],
                                 ref["truncated_seq"], ref["ended_before"], 0.99, 0.95, True)
    assert set(g) == {"advantages", "returns", "valid"}
    RRR.assert_all(f"vec env {backend} gae", g, dict(advantages=adv, returns=ret, valid=valid),
                   ("advantages", "returns", "valid"))
    assert (valid == 0).any() and (valid == 1).any()
    with pytest.raises(ValueError):
        v.rollout(pol, T, repeat=n, spawn_route=np.zeros((T, E), np.int32))  # [T, repeat, E] with a repeat
    v.close(), twin.close()


def test_vec_env_numpy(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch(mev):
    import torch
    assert torch.cuda.is_available()
    _vec_layer(mev, "torch")
