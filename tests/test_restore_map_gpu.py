"""Branching from a snapshot (mev_restore_map, include/marlenv.h): env e takes the state, car
sizes and last outputs of the SNAPSHOT's env env_map[e], -1 leaves it alone.  Checked field by
field against what the snapshot held, then by continuing every copy against an oracle built from
its source env, and end to end as a planner uses it: one root fanned out into all envs, each
rolled out with a plan of its own (mev_step_sequence)."""
import numpy as np
import pytest

import golden_replay as G
import oracle_replay as R
import window_ref as RR
from window_ref import DT, OUT_KEYS

pytestmark = pytest.mark.gpu

MAP12 = [3, 3, 3, 0, -1, 11, 5, 5, -1, 0, 7, 3]


def _handle(mev, E, N, rays, traffic=False, use_team=True, **cfg):
    """A handle (team reward unless said otherwise) on the tests' routes, reset; and its traffic-route ids."""
    h = RR.handle(mev, E, N, rays, traffic=traffic, use_team=use_team, **cfg)
    return h, RR.set_routes(h, traffic)[1]


def _snap_all(h):
    """State, outputs and car sizes as host copies."""
    return ({k: v.copy() for k, v in h.get_state().items()}, {k: v.copy() for k, v in h.get_outputs().items()},
            tuple(x.copy() for x in h.car_dims()))


def _restore(h, snap, env_map, device):
    if device:
        import torch
        torch.cuda.set_device(0)
        tsnap, tmap = torch.as_tensor(snap).cuda(), torch.as_tensor(np.asarray(env_map, np.int32)).cuda()
        h.restore(tsnap, env_map=tmap, device=True)
        h.sync()  # (the tensors stay alive until the handle's stream is done)
    else:
        h.restore(snap, env_map=env_map)


def _check_copy(tag, got, src, before, env_map):
    """Env e of `got` equals env env_map[e] of `src` (the snapshot-time values), or, where the map
    says -1, env e of `before` (the values right before the restore) -- every array, bit for bit."""
    for part, (g, s, b) in enumerate(zip(got, src, before)):
        items = g.items() if isinstance(g, dict) else enumerate(g)
        for k, v in items:
            for e, m in enumerate(env_map):
                want = b[k][e] if m < 0 else s[k][m]
                assert G.bits_equal(v[e], want), f"{tag}: part {part} field {k} env {e} (map {m})"


def _continue(tag, h, meta, src_state, src_dims, before_state, before_dims, env_map, traffic_routes=None, dims=False,
              seed=21):
    """One oracle per env from the SOURCE env's state; 10 plain steps and one plan rollout must
    match it on every output (spawns replayed in traffic mode, no auto-reset)."""
    E, N = h.E, h.N
    oracles = []
    for e, m in enumerate(env_map):
        st, dm, i = (before_state, before_dims, e) if m < 0 else (src_state, src_dims, m)
        oracles.append(R.oracle_from_device_state(meta, st, i, traffic_routes, dm if dims else None))
    ref = RR.WindowRef(oracles, np.zeros((E, N), np.int32))
    rng = np.random.default_rng(seed)
    traffic = traffic_routes is not None
    for t in range(10):
        A, _, sp = RR.draw_plan(rng, E, N, 1, 0.5, traffic)
        out = h.step(A[0], DT, spawn_route=None if sp is None else sp[0])
        ws = ref.step(A, [DT], sp, auto_reset=False)
        st = h.get_state()
        cd = h.car_dims() if dims else None
        for e in range(E):
            R.check_step(f"{tag}: step {t} env {e}", out, e, ws[e])
            R.check_state(f"{tag}: step {t} env {e}", st, e, oracles[e], cd)
    T = 4
    A, dts, sp = RR.draw_plan(rng, E, N, T, 0.5, traffic)
    out = h.step_sequence(A, dts, spawn_route=sp)
    ws = ref.step(A, dts, sp, auto_reset=False)
    st = h.get_state()
    for e in range(E):
        RR.check_window(f"{tag}: plan env {e}", out, e, ws[e], T)
        R.check_state(f"{tag}: plan env {e}", st, e, oracles[e], h.car_dims() if dims else None)
    ref.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_copying_and_continuing(mev, device):
    E, N, rays = 12, 3, 16
    h, _ = _handle(mev, E, N, rays)
    rng = np.random.default_rng(12)
    for t in range(25):  # no auto-reset: the envs drift apart
        h.step(RR.draw(rng, E, N, 0.6)[0], DT)
    src = _snap_all(h)
    assert len({src[0]["x"][e].tobytes() for e in range(E)}) == E  # (the envs differ)
    snap = h.snapshot()
    for t in range(5):
        h.step(RR.draw(rng, E, N, 0.6)[0], DT)
    before = _snap_all(h)
    assert not G.bits_equal(before[0]["x"], src[0]["x"])
    _restore(h, snap, MAP12, device)
    _check_copy("copy", _snap_all(h), src, before, MAP12)
    _continue("continue", h, RR.meta(N, rays, use_team=True), src[0], src[2], before[0], before[2], MAP12)
    h.close()


@pytest.mark.parametrize("dims", [False, True], ids=["54x24", "car_dims"])
def test_traffic_and_car_sizes(mev, dims):
    E, N, rays = 16, 1, 16
    h, ids = _handle(mev, E, N, rays, traffic=True, density=5.0, max_steps=2000, use_team=False)
    rng = np.random.default_rng(13)
    if dims:
        drng = np.random.default_rng(41)
        K = h.K
        h.set_car_dims(np.stack([drng.uniform(40, 70, (E, N)), drng.uniform(18, 30, (E, N))], -1).astype(np.float32),
                       np.stack([drng.uniform(40, 70, (E, K)), drng.uniform(18, 30, (E, K))], -1).astype(np.float32))
    for t in range(40):  # spawns replayed, so every env's traffic is its own: env e tries every (1 + e % 4)-th step
        a, _ = RR.draw(rng, E, N, 0.5)
        sp = rng.integers(-1, 12, E)
        sp[t % (1 + np.arange(E) % 4) != 0] = -1
        h.step(a, DT, spawn_route=sp)
    src = _snap_all(h)
    counts = src[0]["npc_count"]
    print("NPC counts at the snapshot", counts.tolist())
    assert len(set(counts.tolist())) >= 2 and counts.max() >= 1, counts  # (the NPC counts differ between envs)
    snap = h.snapshot()
    for t in range(5):
        a, _ = RR.draw(rng, E, N, 0.5)
        h.step(a, DT, spawn_route=rng.integers(-1, 12, E))
    before = _snap_all(h)
    order = np.argsort(-counts, kind="stable")
    env_map = [int(order[0])] * 5 + [-1, int(order[1]), int(order[-1])] + [int(x) for x in order[:8]]
    assert len(env_map) == E
    _restore(h, snap, env_map, device=False)
    _check_copy("traffic copy", _snap_all(h), src, before, env_map)
    meta = RR.meta(N, rays, traffic=True, density=5.0, use_team=False)
    _continue("traffic continue", h, meta, src[0], src[2], before[0], before[2], env_map, traffic_routes=ids, dims=dims)
    h.close()


def test_errors_leave_the_handle_unchanged(mev):
    E, N, rays = 12, 3, 16
    h, _ = _handle(mev, E, N, rays)
    rng = np.random.default_rng(14)
    for t in range(8):
        h.step(RR.draw(rng, E, N, 0.6)[0], DT)
    src = _snap_all(h)
    snap = h.snapshot()
    for t in range(3):
        h.step(RR.draw(rng, E, N, 0.6)[0], DT)
    before = _snap_all(h)
    for bad in (E, -2):
        m = list(MAP12)
        m[7] = bad
        with pytest.raises(mev.MevError):
            h.restore(snap, env_map=m)
        _check_copy(f"bad entry {bad}", _snap_all(h), before, before, [-1] * E)
    with pytest.raises(ValueError):
        h.restore(snap, env_mask=np.ones(E, np.uint8), env_map=MAP12)
    with pytest.raises(ValueError):
        h.restore(snap, env_map=MAP12[:-1])
    # a snapshot of another shape is refused as by mev_restore
    other, _ = _handle(mev, E, N + 1, rays)
    with pytest.raises(mev.MevError):
        h.restore(other.snapshot(), env_map=MAP12)
    other.close()
    _check_copy("other shape", _snap_all(h), before, before, [-1] * E)
    # device pointers: a bad entry is treated as -1
    import torch
    torch.cuda.set_device(0)
    m = list(MAP12)
    m[7], m[2] = E, -2
    _restore(h, snap, m, device=True)
    m[7] = m[2] = -1
    _check_copy("device bad entries", _snap_all(h), src, before, m)
    h.close()


def test_planner_fan_out_end_to_end(mev):
    """Fork env 0 into all 8 envs, roll each out with a plan of its own: every env equals an
    oracle cloned from env 0's state running that plan; envs given the same plan are bit-identical."""
    E, N, rays, T = 8, 3, 16, 6
    h, _ = _handle(mev, E, N, rays, max_steps=2000)
    rng = np.random.default_rng(15)
    for t in range(20):
        h.step(RR.draw(rng, E, N, 0.6)[0], DT)
    root = _snap_all(h)
    snap = h.snapshot()
    h.restore(snap, env_map=np.zeros(E, np.int32))
    A, dts, _ = RR.draw_plan(rng, E, N, T, 0.6)
    A[:, 5] = A[:, 2]  # envs 2, 5 and 7 evaluate the same plan
    A[:, 7] = A[:, 2]
    out = h.step_sequence(A, dts)
    st = h.get_state()
    meta = RR.meta(N, rays, use_team=True)
    for e in range(E):
        o = R.oracle_from_device_state(meta, root[0], 0)
        w = RR.window_step(o, A[:, e], dts)
        RR.check_window(f"fan-out env {e}", out, e, w, T)
        R.check_state(f"fan-out env {e}", st, e, o)
        o.close()
    for e in (5, 7):
        for k in OUT_KEYS + ("substeps",):
            assert G.bits_equal(out[k][e], out[k][2]), (e, k)
        for k in ("reward_seq", "done_seq", "status_seq"):
            assert G.bits_equal(out[k][:, e], out[k][:, 2]), (e, k)
        for k in st:
            assert G.bits_equal(st[k][e], st[k][2]), (e, k)
    assert not G.bits_equal(out["reward_seq"][:, 0], out["reward_seq"][:, 1])  # (different plans differ)
    h.close()
