"""mev_evaluate_leaves (include/marlenv.h): mev_evaluate_plans plus, for every candidate, the
observation of the state it stopped at.  leaf_obs[c] is checked bit for bit against the `obs` of the
window contract (window_ref.window_step) run on an oracle built from the root env's device state,
every other output against mev_evaluate_plans on the same inputs, and the handle must stay as it
was.  The scenarios are those of tests/test_evaluate_plans_gpu.py (its histories, plans and helpers
are imported, not copied) plus the ones each test names; every output buffer is filled with 0xFF
bytes before the call, so a float the call does not write shows.

The seeds were chosen on the CPU with the oracle alone (the histories replayed by oracles), so that
each coverage assertion below holds for the oracle by construction:
 - scenario 1 (PLAIN): sub-step counts [1, 1, 1, 5, 5, 3, 1, 5, 5, 5, 1, 3, 5], one crash with a
   respawn before a plan's last sub-step;
 - the car pair: plan seed 60 on root 2, agent 1's actions replaced -- agent 2's own pose columns
   are the same in both leaves and 5 of its 16 beams differ;
 - respawn off: the reference never clears Car::alive, so the dead agents are written into the
   roots with mev_set_state."""
import ctypes

import numpy as np
import pytest

import golden_replay as G
import oracle_replay as R
import test_evaluate_plans_gpu as EP
import window_ref as RR
from test_evaluate_plans_gpu import ALL, PLAIN, ROOTS13, SEQ, TRAFFIC, TWELVE
from window_ref import CRASH_CAR, DT

pytestmark = pytest.mark.gpu

HEAD = 31  # columns of the observation head; the LiDAR block follows
# the scoring call's outputs: dtype and shape of (T, C, N)
OUTS = dict(returns=(np.float32, lambda T, C, N: (C, N)), reward_seq=(np.float32, lambda T, C, N: (T, C, N)),
            done_seq=(np.uint8, lambda T, C, N: (T, C, N)), status_seq=(np.uint8, lambda T, C, N: (T, C, N)),
            substeps=(np.int32, lambda T, C, N: (C,)), terminated=(np.uint8, lambda T, C, N: (C,)),
            truncated=(np.uint8, lambda T, C, N: (C,)))


def filled(shape, dtype):
    """An output buffer of 0xFF bytes."""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xFF
    return a


def outputs(T, C, N, D=None):
    o = {k: filled(shape(T, C, N), dtype) for k, (dtype, shape) in OUTS.items()}
    if D is not None:
        o["leaf_obs"] = filled((C, N, D), np.float32)
    return o


def both(h, A, roots, dts, gamma, spawn_route=None):
    """(the leaf call's outputs, mev_evaluate_plans' on the same inputs), every buffer prefilled."""
    T, C, N = A.shape[0], A.shape[1], h.N
    leaf = h.evaluate_plans(A, roots, dts, gamma, spawn_route=spawn_route, out=outputs(T, C, N, h.D), leaf_obs=True)
    plain = h.evaluate_plans(A, roots, dts, gamma, spawn_route=spawn_route, out=outputs(T, C, N))
    return leaf, plain


def reference(meta, state, roots, A, dts, sp=None, traffic_routes=None, dims=None, rel=None):
    """Each candidate's window from an oracle holding its root's state (rel: a written beam list)."""
    ws = []
    for c, r in enumerate(roots):
        o = R.oracle_from_device_state(meta, state, int(r), traffic_routes, dims)
        if rel is not None:
            o.set_rel_angles(rel)
        ws.append(RR.window_step(o, A[:, c], dts, None if sp is None else sp[:, c]))
        o.close()
    return ws


def no_fill_left(tag, leaf):
    assert not (leaf.view(np.uint32) == 0xFFFFFFFF).any(), tag + ": a float of leaf_obs was not written"


def check_leaves(tag, leaf, plain, ws):
    """leaf_obs against the oracles' leaf rows, everything else against the scoring call."""
    for c, w in enumerate(ws):
        assert G.bits_equal(leaf["leaf_obs"][c], w["obs"]), f"{tag}: leaf_obs of candidate {c} (k = {w['substeps']})"
    for k in ALL:
        assert G.bits_equal(leaf[k], plain[k]), f"{tag}: {k} differs from mev_evaluate_plans"
    no_fill_left(tag, leaf["leaf_obs"])


def crash_before_last(ws):
    """sub-steps with a crash (and so, with respawn on, a respawn) that are not the candidate's last"""
    return sum(int(((r["done"] != 0) & (r["status"] >= RR.CRASH_WALL)).any()) for w in ws for r in w["sub"][:-1])


# ---- scenario 1 (shared: computed once, never changed) ----

@pytest.fixture(scope="module")
def plain(mev):
    P = PLAIN
    h, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
    EP._device_history_plain(h, P["seed"])
    before = EP._snap_all(h)
    A, dts = EP.plans_plain(np.random.default_rng(P["plan_seed"]), P["N"], ROOTS13, P["T"])
    leaf, scored = both(h, A, ROOTS13, dts, P["gamma"])
    after = EP._snap_all(h)
    ws = reference(RR.meta(P["N"], P["rays"], **P["cfg"]), before["state"], ROOTS13, A, dts)
    yield dict(h=h, A=A, dts=dts, leaf=leaf, scored=scored, ws=ws, before=before, after=after)
    h.close()


def test_oracle_no_traffic(mev, plain):
    P, S = PLAIN, plain
    ws, T = S["ws"], P["T"]
    ks = [w["substeps"] for w in ws]
    print("substeps", ks, "crashes before a plan's last sub-step", crash_before_last(ws))
    assert sum(k < T for k in ks) >= 3 and any(1 < k < T for k in ks)
    assert crash_before_last(ws) >= 1  # (a respawn inside a plan: the leaf is cast from the respawned state)
    assert S["h"].D == 127 and S["leaf"]["leaf_obs"].shape == (13, P["N"], 127)  # (padding columns beyond 31 + 16)
    check_leaves("scenario 1", S["leaf"], S["scored"], ws)
    for c in range(len(ROOTS13)):
        EP.check_candidate(f"candidate {c}", S["leaf"], c, ws[c], T, P["gamma"])
    assert not S["leaf"]["leaf_obs"][:, :, HEAD + P["rays"]:].view(np.uint32).any()  # the padding: zero bits


def test_car_pair_hits(mev, plain):
    """Two candidates of root 2 whose plans differ only in agent 1's actions: agent 2's own pose is the
    same in both leaves, its LiDAR block is not -- a difference only agent 1's box can make."""
    P, S = PLAIN, plain
    h, r, j, i = S["h"], 2, 1, 2
    A1, dts, _ = RR.draw_plan(np.random.default_rng(60), 1, P["N"], P["T"], 0.6)
    A2 = A1.copy()
    A2[:, 0, j, 0] = -1.0
    A2[:, 0, j, 1] = -A1[:, 0, j, 1]
    A = np.concatenate([A1, A2], 1)
    others = [a for a in range(P["N"]) if a != j]
    assert G.bits_equal(A[:, 0, others], A[:, 1, others])
    ws = reference(RR.meta(P["N"], P["rays"], **P["cfg"]), S["before"]["state"], [r, r], A, dts)
    o1, o2 = ws[0]["obs"][i], ws[1]["obs"][i]
    assert o1[:4].any() and G.bits_equal(o1[:4], o2[:4])            # (the oracle: same own x, y, v, heading ...
    assert not G.bits_equal(o1[HEAD:HEAD + P["rays"]], o2[HEAD:HEAD + P["rays"]])  # ... another LiDAR block)
    leaf, scored = both(h, A, [r, r], dts, P["gamma"])
    check_leaves("car pair", leaf, scored, ws)
    g1, g2 = leaf["leaf_obs"][0, i], leaf["leaf_obs"][1, i]
    assert G.bits_equal(g1[:4], g2[:4]) and not G.bits_equal(g1[HEAD:HEAD + P["rays"]], g2[HEAD:HEAD + P["rays"]])


def test_equals_restore_map_and_step_sequence(mev):
    """C == E, plain rows of 31 + R columns: leaf_obs is the obs of restore(env_map=roots) + step_sequence."""
    E = C = N = 8
    rays, T = 64, 5
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=rays, obs_dim=0, use_team_reward=1, respawn_enabled=1,
                   max_steps=2000, seed=7, device=0)
    RR.set_routes(h)
    assert h.D == HEAD + rays
    EP._device_history_plain(h, 41, steps=20, reset_at={})
    before = EP._snap_all(h)
    rng = np.random.default_rng(42)
    roots = np.array([3, 3, 0, 7, 1, 0, 5, 3], np.int32)
    A, dts, _ = RR.draw_plan(rng, C, N, T, 0.6)
    leaf, scored = both(h, A, roots, dts, 0.9)
    EP._assert_same("C == E", before, EP._snap_all(h))
    snap = h.snapshot()
    h.restore(snap, env_map=roots)
    seq = h.step_sequence(A, dts)
    assert G.bits_equal(leaf["leaf_obs"], seq["obs"])
    for k in SEQ + ("substeps",):
        assert G.bits_equal(leaf[k], seq[k]), k
    for k in ALL:
        assert G.bits_equal(leaf[k], scored[k]), k
    no_fill_left("C == E", leaf["leaf_obs"])
    assert len({leaf["leaf_obs"][c].tobytes() for c in range(C)}) >= 5  # (five different roots: not one row repeated)
    h.restore(snap)
    st = h.get_state()
    for k in st:
        assert G.bits_equal(st[k], before["state"][k]), k
    h.close()


def test_twelve_agents_and_car_sizes(mev):
    P = TWELVE
    E, N, T, C = P["E"], P["N"], P["T"], P["C"]
    h, _ = EP._handle(mev, E, N, P["rays"], **P["cfg"])
    drng = np.random.default_rng(40)
    h.set_car_dims(np.stack([drng.uniform(40, 70, (E, N)), drng.uniform(18, 30, (E, N))], -1).astype(np.float32), None)
    EP._device_history_plain(h, P["seed"], steps=12, reset_at={})
    assert h.car_dims_active()
    before = EP._snap_all(h)
    roots = [3, 0, 0, 2, 1, 3, 3, 2, 0]
    A, dts, _ = RR.draw_plan(np.random.default_rng(P["seed"] + 1), C, N, T, 0.6)
    leaf, scored = both(h, A, roots, dts, P["gamma"])
    EP._assert_same("twelve agents", before, EP._snap_all(h))
    ws = reference(RR.meta(N, P["rays"], **P["cfg"]), before["state"], roots, A, dts, dims=before["dims"])
    check_leaves("twelve agents", leaf, scored, ws)
    assert crash_before_last(ws) >= 1
    h.close()


@pytest.mark.parametrize("max_npcs", [32, 64])
def test_traffic_spawn_replay(mev, max_npcs):
    P = TRAFFIC
    h, ids, roots, A, dts, sp = EP._traffic(mev, max_npcs)
    before = EP._snap_all(h)
    counts = before["state"]["npc_count"]
    assert len(set(counts[roots].tolist())) >= 2 and counts.max() >= 3, counts
    leaf, scored = both(h, A, roots, dts, P["gamma"], spawn_route=sp)
    EP._assert_same("traffic", before, EP._snap_all(h))
    ws = reference(RR.meta(P["N"], P["rays"], **P["cfg"]), before["state"], roots, A, dts, sp, traffic_routes=ids)
    assert any(((r["done"] != 0) & (r["status"] == CRASH_CAR)).any() for w in ws for r in w["sub"])
    check_leaves(f"traffic, {max_npcs} slots", leaf, scored, ws)
    h.close()


def test_respawn_disabled_dead_agents(mev):
    """Dead agents at the leaf: their rows are zero, their boxes still obstacles of the others' beams."""
    E, N, rays, T = 6, 3, 16, 5
    cfg = dict(use_team=True, respawn=False, max_steps=2000)
    h, _ = EP._handle(mev, E, N, rays, **cfg)
    EP._device_history_plain(h, 52, steps=25, reset_at={})
    st = h.get_state()
    st["alive"][0, 1] = 0
    st["alive"][3, 0] = 0
    st["alive"][3, 2] = 0
    h.set_state(st)
    before = EP._snap_all(h)
    A, dts, _ = RR.draw_plan(np.random.default_rng(53), 13, N, T, 0.6)
    leaf, scored = both(h, A, ROOTS13, dts, 0.97)
    EP._assert_same("respawn off", before, EP._snap_all(h))
    ws = reference(RR.meta(N, rays, **cfg), before["state"], ROOTS13, A, dts)
    check_leaves("respawn off", leaf, scored, ws)
    dead = [(c, i) for c, r in enumerate(ROOTS13) for i in range(N) if before["state"]["alive"][r, i] == 0]
    assert len(dead) >= 5 and any(w["substeps"] > 1 for w in ws)
    for c, i in dead:
        assert not ws[c]["obs"][i].view(np.uint32).any() and not leaf["leaf_obs"][c, i].view(np.uint32).any(), (c, i)
    h.close()


def test_beam_list_without_culling(mev):
    """An uneven beam list: every beam is resolved against every candidate box, no angular culling."""
    P = PLAIN
    rel = np.sort(np.random.default_rng(1).uniform(-np.pi, np.pi, P["rays"])).astype(np.float32)
    assert len(set(np.diff(rel).round(4).tolist())) > 4  # (uneven)
    h, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
    h.set_beam_angles(rel)
    EP._device_history_plain(h, P["seed"])
    before = EP._snap_all(h)
    A, dts = EP.plans_plain(np.random.default_rng(P["plan_seed"]), P["N"], ROOTS13, P["T"])
    leaf, scored = both(h, A, ROOTS13, dts, P["gamma"])
    EP._assert_same("uneven beams", before, EP._snap_all(h))
    ws = reference(RR.meta(P["N"], P["rays"], **P["cfg"]), before["state"], ROOTS13, A, dts, rel=rel)
    check_leaves("uneven beams", leaf, scored, ws)
    h.close()


def test_chunks(mev, plain, monkeypatch):
    """MEV_LEAF_CHUNK=4 at creation: 13 candidates in chunks of 4, 4, 4 and 1, every output the same."""
    P, S = PLAIN, plain
    monkeypatch.setenv("MEV_LEAF_CHUNK", "4")
    h, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
    monkeypatch.delenv("MEV_LEAF_CHUNK")
    EP._device_history_plain(h, P["seed"])
    leaf, _ = both(h, S["A"], ROOTS13, S["dts"], P["gamma"])
    for k in ALL + ("leaf_obs",):
        assert G.bits_equal(leaf[k], S["leaf"][k]), k
    EP._assert_same("chunks", S["before"], EP._snap_all(h))
    h.close()


def test_device_pointers(mev, plain):
    import torch
    torch.cuda.set_device(0)
    P, S = PLAIN, plain
    h, T, N, C, D = S["h"], P["T"], P["N"], len(ROOTS13), S["h"].D
    dev = "cuda:0"

    def garbage():
        return {k: torch.as_tensor(v).to(dev) for k, v in outputs(T, C, N, D).items()}

    tA = torch.as_tensor(S["A"]).to(dev).contiguous()

    def call(roots, o):
        h.evaluate_plans(tA, torch.as_tensor(np.asarray(roots, np.int32)).to(dev), S["dts"], P["gamma"], out=o,
                         device=True, leaf_obs=True)
        h.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    got = call(ROOTS13, garbage())
    for k in ALL + ("leaf_obs",):
        assert G.bits_equal(got[k], S["leaf"][k]), k
    # roots outside [0, E): those candidates are all zero bits, their neighbours unchanged
    bad = list(ROOTS13)
    bad[4], bad[9] = P["E"], -1
    got = call(bad, garbage())
    for k in ALL + ("leaf_obs",):
        want = S["leaf"][k].copy()
        if k in SEQ:
            want[:, [4, 9]] = 0
        else:
            want[[4, 9]] = 0
        assert G.bits_equal(got[k], want), k
    # only leaf_obs: nothing else is written
    o = garbage()
    got = call(ROOTS13, dict(leaf_obs=o["leaf_obs"]))
    assert G.bits_equal(got["leaf_obs"], S["leaf"]["leaf_obs"])
    for k in ALL:
        assert (o[k].cpu().numpy().view(np.uint8) == 0xFF).all(), k
    EP._assert_same("device calls", S["before"], EP._snap_all(h))


def test_handle_untouched_no_traffic(mev, plain):
    P, S = PLAIN, plain
    EP._assert_same("scenario 1", S["before"], S["after"])

    def twin():
        t, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
        EP._device_history_plain(t, P["seed"])
        return t

    h = twin()  # (a copy: the shared scenario's handle stays where the other tests expect it)
    leaf, _ = both(h, S["A"], ROOTS13, S["dts"], P["gamma"])
    assert G.bits_equal(leaf["leaf_obs"], S["leaf"]["leaf_obs"])
    EP._twin_step("scenario 1", mev, h, twin, P["N"])
    h.close()


def test_handle_untouched_traffic(mev):
    P = TRAFFIC
    h, ids, roots, A, dts, sp = EP._traffic(mev, 32)
    before = EP._snap_all(h)
    T, C = A.shape[0], A.shape[1]
    h.evaluate_plans(A, roots, dts, P["gamma"], spawn_route=sp, out=outputs(T, C, h.N, h.D), leaf_obs=True)
    o = h.evaluate_plans(A, roots, dts, P["gamma"], out=outputs(T, C, h.N, h.D), leaf_obs=True)  # (the Philox spawner)
    no_fill_left("philox", o["leaf_obs"])
    EP._assert_same("traffic", before, EP._snap_all(h))

    def twin():
        t, _ = EP._handle(mev, P["E"], P["N"], P["rays"], max_npcs=32, **P["cfg"])
        EP._device_history_traffic(t, P["seed"])
        return t

    EP._twin_step("traffic", mev, h, twin, P["N"])
    h.close()


def test_errors(mev):
    E, N, rays, T, C = 2, 1, 16, 3, 2
    cfg = dict(use_team=False, max_steps=0)
    meta = RR.meta(N, rays, **cfg)

    def make():
        t, _ = EP._handle(mev, E, N, rays, **cfg)
        EP._device_history_plain(t, 35, steps=5, reset_at={})
        return t

    h, twin = make(), make()
    rng = np.random.default_rng(36)
    A, dts, _ = RR.draw_plan(rng, C, N, T, 0.6)
    L = mev._capi

    def step_as_twin(tag):
        """h is where its twin (which never makes the call) is, and the two step on alike."""
        a, _ = RR.draw(rng, E, N, 0.5)
        sa, sb = EP._snap_all(h), EP._snap_all(twin)
        oa, ob = h.step(a, DT), twin.step(a, DT)
        for part in ("state", "outputs"):
            for k in sa[part]:
                assert G.bits_equal(sa[part][k], sb[part][k]), f"{tag}: {part} {k}"
        assert sa["npc_stats"] == sb["npc_stats"], tag
        for k in RR.OUT_KEYS:
            assert G.bits_equal(oa[k], ob[k]), f"{tag}: {k} of the next step"

    # null leaf_obs (the wrapper would allocate one: the raw call)
    la = L.MevLeafArgs()
    roots = np.array([0, 1], np.int32)
    ret = filled((C, N), np.float32)
    la.eval.actions, la.eval.roots, la.eval.returns = A.ctypes.data, roots.ctypes.data, ret.ctypes.data
    la.eval.candidates, la.eval.length, la.eval.dt, la.eval.gamma = C, T, DT, 0.9
    assert h._lib.mev_evaluate_leaves(h._h, ctypes.byref(la)) == -1
    assert b"leaf_obs" in h._lib.mev_last_error()
    assert (ret.view(np.uint8) == 0xFF).all()
    step_as_twin("null leaf_obs")
    # only leaf_obs, every output of `eval` null
    only = h.evaluate_plans(A, roots, dts, 0.9, out=dict(leaf_obs=filled((C, N, h.D), np.float32)), leaf_obs=True)
    assert set(only) == {"leaf_obs"}
    ws = reference(meta, h.get_state(), roots, A, dts)
    for c in range(C):
        assert G.bits_equal(only["leaf_obs"][c], ws[c]["obs"]), c
    step_as_twin("only leaf_obs")
    with pytest.raises(L.IndexRangeError):
        h.evaluate_plans(A, [0, E], dts, 0.9, leaf_obs=True)
    with pytest.raises(mev.MevError):
        h.evaluate_plans(A, [-1, 0], dts, 0.9, leaf_obs=True)
    step_as_twin("root out of range")
    with pytest.raises(mev.MevError) as exc:
        h.evaluate_plans(A, roots, dts, 0.9, flags=L.MEV_AUTO_RESET, leaf_obs=True)
    assert not isinstance(exc.value, L.IndexRangeError)
    step_as_twin("a flag other than MEV_DEVICE_PTRS")
    for bad_A, bad_roots in ((np.zeros((T, 0, N, 2), np.float32), np.zeros(0, np.int32)),
                             (np.zeros((L.MEV_MAX_REPEAT + 1, C, N, 2), np.float32), roots)):
        with pytest.raises(mev.MevError):
            h.evaluate_plans(bad_A, bad_roots, DT, leaf_obs=True)
    step_as_twin("refused shapes")
    h.close()
    twin.close()


def _vec_layer(mev, backend):
    import pkgload
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, rays, T, C = 4, 2, 16, 3, 6
    v = vec_env.VecIntersectionEnv(E, N, lidar_rays=rays, use_team_reward=True, max_steps=10, backend=backend)
    RR.set_routes(v.handle)
    rng = np.random.default_rng(9)
    for call in range(2):
        for t in range(2):
            v.step(RR.draw(rng, E, N, 0.6)[0])
        state = {k: x.copy() for k, x in v.handle.get_state().items()}
        roots = rng.integers(0, E, C).astype(np.int32)
        A, dts, _ = RR.draw_plan(rng, C, N, T, 0.6)
        default = v.evaluate_plans(A, roots, dt=dts, gamma=0.9)
        assert set(default) == set(ALL)  # (no "leaf_obs" key)
        out = v.evaluate_plans(A, roots, dt=dts, gamma=0.9, leaf_obs=True)
        assert set(out) == set(ALL) | {"leaf_obs"}
        assert set(v.evaluate_plans(A, roots, dt=dts, gamma=0.9)) == set(ALL)  # (nor after a leaf call)
        if backend == "torch":
            assert out["leaf_obs"].is_cuda
            out = {k: x.cpu().numpy() for k, x in out.items()}
        D = v.handle.D
        want = v.handle.evaluate_plans(A, roots, dts, 0.9, out=outputs(T, C, N, D), leaf_obs=True)
        for k in ALL + ("leaf_obs",):
            assert G.bits_equal(out[k], want[k]), (backend, call, k)
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
