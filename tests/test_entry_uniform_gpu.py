"""Phase 1's entry bound specialised by the road region of the car centre
(road_entry_safe_uniform, csrc/mev_roadbound.h) in the one-wave k_step kernels whose phase 1 is the
branch-free agent-pair loop: 8 x 64 beams (the metric's instantiation, one pass per agent) and
8 x 128 beams (config 5's, two passes per agent), the split off as at 4096 envs.

(a) Cars planted in every region -- the centre cross, both arms, a corner fillet, and within one
    pixel of the |r| = rwm lines the regions are cut along, in each axis -- with headings over the
    whole circle and on the axes, zero speed, one step with zero actions and respawn off: the
    observation rows against the C oracle (oracle/marl_oracle.c), bit for bit.
(b) 200 random steps with auto-reset: every output of every step against a second handle on
    k_cars + k_lidar, which marches with road_safe, an independent bound."""
import numpy as np
import pytest

import golden_replay as G
import oracle_replay as ORP

pytestmark = pytest.mark.gpu

N, RW, CR = 8, 126.0, 84.0  # three lanes: the road's half width, the corner radius
RWM = np.float32(RW - 1.5)  # the regions' border (mev_roadbound.h)
SHAPES = [dict(rays=64, envs=64), dict(rays=128, envs=32)]
IDS = ["8x64", "8x128"]
REGIONS = ["cross", "vertical arm", "horizontal arm", "general"]


def _fused(mev, shape, **cfg):
    h = mev.Handle(num_envs=shape["envs"], num_agents=N, lidar_rays=shape["rays"], **cfg)
    h.set_step_split(1)  # one wave per env, as at 4096 envs
    assert h.step_kernel() == 2 and h.step_split() == 0 and h.step_pack() == 1
    return h


def _planted(rng, E):
    """x, y, heading [E][N]: env e's cars in region e % 4, its cars 0 and 1 within one pixel of
    |rx| = rwm and |ry| = rwm; the fillet cars between the arms' corner and the grass disc."""
    x, y = np.empty((E, N)), np.empty((E, N))
    sgn = lambda: rng.choice([-1.0, 1.0], N)  # noqa: E731
    for e in range(E):
        inside = lambda: rng.uniform(-(RW - 3.0), RW - 3.0, N)  # noqa: E731
        along = lambda: sgn() * rng.uniform(RW, 370.0, N)  # noqa: E731
        fillet = lambda: sgn() * rng.uniform(RW - 1.5, RW + 12.0, N)  # noqa: E731
        rx, ry = [(inside(), inside()), (inside(), along()), (along(), inside()), (fillet(), fillet())][e % 4]
        rx[0] = rng.choice([-1.0, 1.0]) * (RW - 1.5 + rng.uniform(-1.0, 1.0))
        ry[1] = rng.choice([-1.0, 1.0]) * (RW - 1.5 + rng.uniform(-1.0, 1.0))
        x[e], y[e] = 375.0 + rx, 375.0 + ry
    hd = rng.uniform(-np.pi, np.pi, (E, N))
    hd[:, 2:6] = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi])  # on the axes, in every region's envs
    return x, y, hd


def _region(x, y):
    """The region test of road_entry_safe_uniform on the float32 poses the handle holds."""
    xin = np.abs(x.astype(np.float32) - np.float32(375.0)) < RWM
    yin = np.abs(y.astype(np.float32) - np.float32(375.0)) < RWM
    return np.where(xin & yin, 0, np.where(xin, 1, np.where(yin, 2, 3)))


def _oracle_obs(shape, st, e, D):
    o = ORP.O.OracleEnv(num_lanes=3, n_agents=N, rays=shape["rays"], obs_dim=D, respawn=False)
    cars = ORP.O.new_cars(N)
    for a, b in ORP.EGO_FIELDS.items():
        cars[a] = st[b][e]
    o.set_state(cars, ORP.O.new_cars(0), int(st["step_count"][e]))
    r = o.step(np.zeros((N, 2), np.float32), 1.0 / 60.0, -1)
    o.close()
    return r["obs"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_each_region_matches_the_oracle(mev, shape):
    E, R_ = shape["envs"], shape["rays"]
    rng = np.random.default_rng(41 + R_)
    h = _fused(mev, shape, respawn_enabled=0)
    try:
        st = h.get_state()
        st["x"][:], st["y"][:], st["heading"][:] = _planted(rng, E)
        st["alive"][:] = 1
        for f in ("v", "acc", "steering"):
            st[f][:] = 0.0
        h.set_state(st)
        st = h.get_state()
        reg = _region(st["x"], st["y"])
        counts = [int((reg == k).sum()) for k in range(4)]
        print("agents per region:", dict(zip(REGIONS, counts)))
        assert min(counts) >= 32, counts
        # within one pixel of the border, on both of its sides, in each axis
        for c in ("x", "y"):
            d = np.abs(st[c].astype(np.float32) - np.float32(375.0)) - RWM
            assert ((d > -1.0) & (d < 0.0)).any() and ((d >= 0.0) & (d < 1.0)).any(), c
        for hd in (0.0, np.pi / 2, -np.pi / 2, np.pi):
            for k in range(4):  # a zero direction component through every region's block
                assert ((st["heading"] == np.float32(hd)) & (reg == k)).any(), (hd, REGIONS[k])
        got = h.step(np.zeros((E, N, 2), np.float32))["obs"]
        for e in range(E):
            want = _oracle_obs(shape, st, e, h.D)
            if not G.bits_equal(got[e], want):
                bad = np.argwhere(got[e].view(np.uint32) != want.view(np.uint32))
                i, c = bad[0]
                raise AssertionError(
                    f"env {e}: {len(bad)} words differ, first agent {i} ({REGIONS[reg[e, i]]}) col {c}: got "
                    f"{got[e][i, c]!r} want {want[i, c]!r}; pose "
                    f"{(float(st['x'][e, i]), float(st['y'][e, i]), float(st['heading'][e, i]))}; "
                    f"differing (agent, col): {bad[:12].tolist()}")
        lid = got[:, :, 31:31 + R_]
        stopped = ((lid > 0) & (lid < 1.0)).any(axis=2)
        for k in range(4):  # not vacuous: beams stopped in every region
            assert (stopped & (reg == k)).any(), REGIONS[k]
    finally:
        h.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rollout_equals_the_two_kernel_path(mev, shape):
    E, T = shape["envs"], 200
    cfg = dict(use_team_reward=1, respawn_enabled=1, max_steps=40, seed=13)
    ha = _fused(mev, shape, **cfg)
    hb = mev.Handle(num_envs=E, num_agents=N, lidar_rays=shape["rays"], **cfg)
    hb.set_step_kernel(1)  # k_cars + k_lidar: road_safe
    assert hb.step_kernel() == 1
    rng = np.random.default_rng(17)
    seen = np.zeros(4, np.int64)
    resets = 0
    ended = np.zeros(E, bool)
    try:
        for t in range(T):
            a = rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)
            a[..., 0] = rng.uniform(0.5, 1.0, (E, N)).astype(np.float32)  # throttle: the cars get somewhere
            oa = {k: np.array(v) for k, v in ha.step(a, auto_reset=True).items()}
            ob = hb.step(a, auto_reset=True)
            assert set(oa) == set(ob)
            for k in oa:
                assert np.array_equal(_bits(oa[k]), _bits(ob[k])), (t, k)
            now = (oa["terminated"] != 0) | (oa["truncated"] != 0)
            resets += int((ended & (oa["step"] == 1)).sum())
            ended = now
            if (t + 1) % 20 == 0:
                sa, sb = ha.get_state(), hb.get_state()
                assert set(sa) == set(sb)
                for k in sa:
                    assert np.array_equal(_bits(sa[k]), _bits(sb[k])), (t, k)
                alive = sa["alive"] != 0
                seen += np.bincount(_region(sa["x"], sa["y"])[alive], minlength=4)
    finally:
        ha.close()
        hb.close()
    print("alive agents per region at the sampled steps:", dict(zip(REGIONS, seen.tolist())), "resets:", resets)
    assert resets >= E, resets
    # the episodes are short, so the cars stay in the arms they spawn in: both arms' bodies ran (the
    # cross and the fillets are test (a)'s)
    assert seen[1] > 0 and seen[2] > 0, seen
