"""Plan rollouts (mev_step_sequence, include/marlenv.h) against the oracle: one call that runs a
different action, dt and spawn decision per sub-step and casts the LiDAR once must equal the
reference's step looped over the plan (tests/window_ref.py) -- every output, the sub-step
count, every per-step row and the full state after every call, bit for bit per env.  Each
scenario asserts on the oracle side that it reached the cases it is about (dones inside a plan,
plans stopped early, every crash status), so it cannot pass by covering nothing.  The actions
of one call vary around a shared base, so the reward's smoothness term between sub-steps -- which
a held action never exercises -- is non-zero in every scenario."""
import numpy as np
import pytest

import golden_replay as G
import oracle_replay as R
import window_ref as RR
from window_ref import DT, OUT_KEYS, handle as _handle, start as _start

pytestmark = pytest.mark.gpu

SEQ_KEYS = ("reward_seq", "done_seq", "status_seq")


def _scenario(mev, T, **kw):
    return RR.scenario(mev, n=T, plan=True, **kw)


def test_respawn_on_team_reward(mev):
    ref = _scenario(mev, E=24, N=3, rays=32, T=5, calls=30, seed=3, bias=0.6, use_team=True, max_steps=23)
    print("mid-plan dones", ref.mid_dones, "early stops", ref.early_stops, "resets", ref.resets, ref.status_count)
    assert ref.mid_dones >= 10 and ref.early_stops >= 50
    assert all(v > 0 for v in ref.status_count.values())


def test_respawn_off(mev):
    ref = _scenario(mev, E=24, N=3, rays=32, T=4, calls=40, seed=5, bias=0.6, use_team=False, respawn=False,
                    max_steps=200)
    print("early stops", ref.early_stops, ref.status_count)
    assert ref.early_stops >= 20


@pytest.mark.parametrize("dims", [False, True], ids=["54x24", "car_dims"])
def test_runtime_layout_twelve_agents(mev, dims):
    ref = _scenario(mev, E=6, N=12, rays=16, T=6, calls=20, seed=2, bias=0.6, use_team=True, max_steps=50, dims=dims)
    print("mid-plan dones", ref.mid_dones, "early stops", ref.early_stops, ref.status_count)
    assert ref.mid_dones >= 20


@pytest.mark.parametrize("max_npcs", [32, 64])
def test_traffic_spawn_replay(mev, max_npcs):
    ref = _scenario(mev, E=16, N=1, rays=32, T=4, calls=60, seed=11, bias=0.5, traffic=True, density=5.0,
                    max_steps=150, max_npcs=max_npcs)
    print("peak NPCs", ref.peak_npcs, "early stops", ref.early_stops, ref.status_count)
    assert ref.peak_npcs >= 6 and ref.status_count[RR.CRASH_CAR] >= 20 and ref.early_stops >= 8


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_constant_rows_equal_frame_skip(mev, device):
    """Every row equal and no dt list: every shared output, substeps and the state equal
    mev_step_repeat(repeat = T) bit for bit (E = 13: not a multiple of the 8 XCDs the env order
    is dealt over); T = 1 also equals mev_step."""
    E, N, rays = 13, 3, 16
    hs = [_handle(mev, E, N, rays, use_team=True, max_steps=7) for _ in range(3)]
    for h in hs:
        h.set_ego_routes(RR.ego_routes(h.route_id, E, N)[0])
        h.reset()
    a_h, b_h, c_h = hs
    rng = np.random.default_rng(1)
    if device:
        import torch
        torch.cuda.set_device(0)
    stops = 0
    for c in range(20):
        T = (4, 1, 3, 6)[c % 4]
        a, _ = RR.draw(rng, E, N, 0.6)
        A = np.broadcast_to(a, (T, E, N, 2)).copy()
        if device:
            dev = {x: {k: torch.as_tensor(v).cuda() for k, v in a_h.alloc_outputs().items()} for x in "abc"}
            for x in "ab":
                dev[x]["substeps"] = torch.full((E,), -1, dtype=torch.int32, device="cuda:0")
            dev["a"]["reward_seq"] = torch.full((T, E, N), 7.0, dtype=torch.float32, device="cuda:0")
            dev["a"]["done_seq"] = torch.full((T, E, N), 9, dtype=torch.uint8, device="cuda:0")
            dev["a"]["status_seq"] = torch.full((T, E, N), 9, dtype=torch.uint8, device="cuda:0")
            tA, ta = torch.as_tensor(A).cuda(), torch.as_tensor(a).cuda()  # (alive until the handles' streams are done)
            torch.cuda.synchronize()  # (torch's fills are done before the handles' own streams write)
            a_h.step_sequence(tA, DT, out=dev["a"], auto_reset=True, device=True)
            b_h.step_repeat(ta, T, DT, out=dev["b"], auto_reset=True, device=True)
            a_h.sync()
            b_h.sync()
            oa = {k: v.cpu().numpy() for k, v in dev["a"].items()}
            ob = {k: v.cpu().numpy() for k, v in dev["b"].items()}
        else:
            oa = a_h.step_sequence(A, DT, auto_reset=True)
            ob = b_h.step_repeat(a, T, DT, auto_reset=True)
        for k in OUT_KEYS + ("substeps",):
            assert G.bits_equal(oa[k], ob[k]), (c, k)
        sa, sb = a_h.get_state(), b_h.get_state()
        for k in sa:
            assert G.bits_equal(sa[k], sb[k]), (c, k)
        # the rows: written up to each env's stop, zero after it (the arrays came in non-zero in device mode)
        for e in range(E):
            k_e = int(oa["substeps"][e])
            stops += k_e < T
            assert not oa["reward_seq"][k_e:, e].view(np.uint32).any() and not oa["done_seq"][k_e:, e].any() and \
                not oa["status_seq"][k_e:, e].any(), (c, e)
            acc = oa["reward_seq"][0, e].copy()
            for s in range(1, T):
                acc = (acc + oa["reward_seq"][s, e]).astype(np.float32)
            assert G.bits_equal(acc, oa["reward"][e]), (c, e)
            assert G.bits_equal(oa["done_seq"][:k_e, e].max(0), oa["done"][e]), (c, e)
        if T == 1:  # one row: today's step
            if device:
                c_h.restore(a_snap)
                c_h.step(ta, DT, out=dev["c"], auto_reset=True, device=True)
                c_h.sync()
                oc = {k: v.cpu().numpy() for k, v in dev["c"].items()}
            else:
                c_h.restore(a_snap)
                oc = c_h.step(a, DT, auto_reset=True)
            for k in OUT_KEYS:
                assert G.bits_equal(oa[k], oc[k]), (c, k)
            assert G.bits_equal(oa["reward_seq"][0], oc["reward"]) and G.bits_equal(oa["done_seq"][0], oc["done"])
            assert G.bits_equal(oa["status_seq"][0], oc["status"])
            sc = c_h.get_state()
            for k in sa:
                assert G.bits_equal(sa[k], sc[k]), (c, k)
        a_snap = a_h.snapshot()  # (handle C takes handle A's state before a one-row call)
    assert stops >= 10  # (max_steps 7: plans were cut short)
    for h in hs:
        h.close()


def test_philox_and_per_step_dt_equal_single_steps(mev):
    """The on-device spawner and the per-step dt: sub-step s draws with the handle's counter +
    (s - 1) and spawns with probability 1 - expf(-density * dt_s); the call advances the counter by
    T, so for envs that do not end one call leaves the handle exactly where the single steps do
    -- state, outputs and the draws after it."""
    E, N, rays, T = 32, 1, 16, 4
    hs = [_handle(mev, E, N, rays, traffic=True, density=20.0, max_steps=0, seed=5) for _ in range(2)]
    for h in hs:
        routes, ids = RR.ego_routes(h.route_id, E, N)
        h.set_ego_routes(routes)
        h.set_traffic_routes(ids)
        h.reset()
    A_h, B_h = hs
    rng = np.random.default_rng(6)
    for c in range(6):
        A, dts, _ = RR.draw_plan(rng, E, N, T, 0.5)
        oa = A_h.step_sequence(A, dts, auto_reset=True)
        acc = any_done = None
        latched = np.zeros((E, N), np.uint8)
        for s in range(T):
            ob = {k: v.copy() for k, v in B_h.step(A[s], float(dts[s]), auto_reset=True).items()}
            assert not ob["terminated"].any() and not ob["truncated"].any(), (c, s)  # (no env ends here)
            acc = ob["reward"].copy() if s == 0 else (acc + ob["reward"]).astype(np.float32)
            any_done = ob["done"].copy() if s == 0 else any_done | ob["done"]
            latched = np.where(ob["done"] != 0, ob["status"], latched)
            assert G.bits_equal(oa["reward_seq"][s], ob["reward"]), (c, s)
            assert G.bits_equal(oa["done_seq"][s], ob["done"]) and G.bits_equal(oa["status_seq"][s], ob["status"]), (c, s)
        for k in ("obs", "terminated", "truncated", "agents_alive", "step"):
            assert G.bits_equal(oa[k], ob[k]), (c, k)
        assert G.bits_equal(oa["reward"], acc), c
        assert G.bits_equal(oa["done"], any_done), c
        assert G.bits_equal(oa["status"], np.where(any_done != 0, latched, ob["status"])), c
        assert (oa["substeps"] == T).all()
        sa, sb = A_h.get_state(), B_h.get_state()
        for k in sa:
            assert G.bits_equal(sa[k], sb[k]), (c, k)
    assert int(sb["npc_count"].max()) >= 3  # (density 20: the spawner ran)
    a, _ = RR.draw(rng, E, N, 0.5)
    oa, ob = A_h.step(a, DT, auto_reset=True), B_h.step(a, DT, auto_reset=True)  # the counters agree
    for k in OUT_KEYS:
        assert G.bits_equal(oa[k], ob[k]), k
    for h in hs:
        h.close()


def test_interplay_with_server_snapshot_and_errors(mev):
    E, N, rays, T = 2, 2, 16, 3
    meta = RR.meta(N, rays, use_team=True, max_steps=40)
    h = _handle(mev, E, N, rays, use_team=True, max_steps=40)
    ref = _start(h, meta)
    rng = np.random.default_rng(8)

    def plain(tag):
        a, _ = RR.draw(rng, E, N, 0.6)
        out = h.step(a, DT, auto_reset=True)
        ws = ref.step(a[None], [DT])
        for e in range(E):
            R.check_step(f"{tag} env {e}", out, e, ws[e])

    def plan(tag):
        A, dts, _ = RR.draw_plan(rng, E, N, T, 0.6)
        out = h.step_sequence(A, dts, auto_reset=True)
        ws = ref.step(A, dts)
        for e in range(E):
            RR.check_window(f"{tag} env {e}", out, e, ws[e], T)

    plain("served step")
    assert h.serve_stats()["steps"] == 1 and h.serve_stats()["running"]
    plan("plan after a served step")
    assert h.serve_stats()["running"] == 0
    plain("step after the plan")
    # snapshot, plan, restore, the same plan again
    snap = h.snapshot()
    A, dts, _ = RR.draw_plan(rng, E, N, T, 0.6)
    o1 = {k: v.copy() for k, v in h.step_sequence(A, dts, auto_reset=True).items()}
    ws = ref.step(A, dts)
    for e in range(E):
        RR.check_window(f"plan after snapshot env {e}", o1, e, ws[e], T)
    g1 = {k: v.copy() for k, v in h.get_outputs().items()}
    for k in OUT_KEYS:
        assert G.bits_equal(g1[k], o1[k]), k  # (the call's outputs are the handle's last outputs)
    s1 = h.get_state()
    h.restore(snap)
    o2 = h.step_sequence(A, dts, auto_reset=True)
    for k in o1:
        assert G.bits_equal(o1[k], o2[k]), k
    s2 = h.get_state()
    for k in s1:
        assert G.bits_equal(s1[k], s2[k]), k
    # errors leave the handle untouched
    cap = mev._capi.MEV_MAX_REPEAT
    for bad_T, kw in ((0, {}), (cap + 1, {}), (T, dict(gather=True))):
        with pytest.raises(mev.MevError):
            h.step_sequence(np.zeros((bad_T, E, N, 2), np.float32), DT, auto_reset=True, **kw)
    s3 = h.get_state()
    for k in s1:
        assert G.bits_equal(s1[k], s3[k]), k
    plain("step after the refused calls")
    # host-mode shape errors are ValueErrors
    with pytest.raises(ValueError):
        h.step_sequence(np.zeros((T, E, N + 1, 2), np.float32), DT)
    with pytest.raises(ValueError):
        h.step_sequence(np.zeros((T, E, N, 2), np.float32), [DT] * (T + 1))
    with pytest.raises(ValueError):
        h.step_sequence(np.zeros((T, E, N, 2), np.float32), DT, spawn_route=np.zeros((T + 1, E), np.int32))
    h.close()
    ref.close()


MIXED = dict(E=5, N=2, rays=16, calls=24, seed=4, cfg=dict(traffic=True, density=5.0, max_steps=9))


def _mixed_calls(rng, E, N, calls):
    """The calls of test_both_calls_on_one_handle, cycling a plan of 3 rows with a dt per row, a
    frame-skip window of 4, a single step and a plan of 6 rows with one dt: (call, rows or None,
    A [n][E][N][2], dts [n], sp [n][E]), the host call's arguments of a held window being A[0], dts[0]."""
    for c in range(calls):
        T = (3, None, None, 6)[c % 4]
        if T:
            A, dts, sp = RR.draw_plan(rng, E, N, T, 0.5, True)
            if T == 6:
                dts = [DT] * T
        else:
            n = (0, 4, 1, 0)[c % 4]
            a, sp = RR.draw(rng, E, N, 0.5, n, True)
            A, dts = RR.held(a, DT, n)
        yield c, T, A, dts, sp


def test_both_calls_on_one_handle(mev):
    """mev_step_sequence, mev_step_repeat and mev_step in turn on one host-mode traffic handle: the
    staging buffers of actions, spawn routes, sub-step counts and rows are the state the calls share,
    so every output, substeps, the rows and the full state are checked after every call.  (On the
    oracle alone: 30 windows stop early, all at max_steps = 9, and an env holds up to 3 NPCs.)"""
    E, N, rays, cfg = MIXED["E"], MIXED["N"], MIXED["rays"], MIXED["cfg"]
    h = _handle(mev, E, N, rays, max_npcs=32, **cfg)
    ref = _start(h, RR.meta(N, rays, **cfg), traffic=True)
    for c, T, A, dts, sp in _mixed_calls(np.random.default_rng(MIXED["seed"]), E, N, MIXED["calls"]):
        n = len(A)
        if T:
            out = h.step_sequence(A, dts if T == 3 else DT, spawn_route=sp, auto_reset=True)
        elif n > 1:
            out = h.step_repeat(A[0], n, DT, spawn_route=sp, auto_reset=True)
        else:
            out = h.step(A[0], DT, spawn_route=sp[0], auto_reset=True)
        ws = ref.step(A, dts, sp)
        st = h.get_state()
        for e in range(E):
            tag = f"call {c} ({'plan' if T else 'held'}, {n}) env {e}"
            if T or n > 1:
                RR.check_window(tag, out, e, ws[e], T)
            else:
                R.check_step(tag, out, e, ws[e])
            R.check_state(tag, st, e, ref.oracles[e])
        ref.peak_npcs = max(ref.peak_npcs, max(len(o.get_state()[1]) for o in ref.oracles))
    print("early stops", ref.early_stops, "peak NPCs", ref.peak_npcs, "resets", ref.resets)
    assert ref.early_stops >= 5 and ref.peak_npcs >= 2
    h.close()
    ref.close()


def _vec_layer(mev, backend):
    import pkgload
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, rays, T = 4, 2, 16, 3
    meta = RR.meta(N, rays, use_team=True, max_steps=10)
    v = vec_env.VecIntersectionEnv(E, N, lidar_rays=rays, use_team_reward=True, max_steps=10, backend=backend)
    ref = _start(v.handle, meta)
    rng = np.random.default_rng(9)
    for c in range(15):
        A, dts, _ = RR.draw_plan(rng, E, N, T, 0.6)
        obs, rew, term, trunc, info = v.step_sequence(A, dt=dts)
        if backend == "torch":
            obs, rew, term, trunc = (x.cpu().numpy() for x in (obs, rew, term, trunc))
            info = {k: x.cpu().numpy() for k, x in info.items()}
        out = dict(obs=obs, reward=rew, terminated=term, truncated=trunc, **info)
        ws = ref.step(A, dts)
        for e in range(E):
            RR.check_window(f"{backend} call {c} env {e}", out, e, ws[e], T)
    assert ref.early_stops >= 4  # (max_steps 10, plans of 3: the fourth plan of an episode stops at 1)
    v.close()
    ref.close()


def test_vec_env_numpy_step_sequence(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch_step_sequence(mev):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the device")
    _vec_layer(mev, "torch")
