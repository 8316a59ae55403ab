"""LiDAR parity where the road march's bound (csrc/mev_roadbound.h) decides how far a
beam jumps: cars standing within 3 px of every grass edge (half of them on whole
pixels), on the rims of the corner discs (+- 4 px), inside the centre square, off the
road and off the screen, 40 % of them with axis-aligned headings.  Cars are placed with
zero speed and stepped once with zero actions and respawn off (as in
tests/test_lidar_stress_gpu.py); that step's observation is compared bit for bit with
the C restatement's (oracle/marl_oracle.c), in the smallest shapes that reach each
LiDAR kernel: the metric's one-wave k_step (8 x 64 beams, the split off), its two-wave
split, the 128-beam kernel (two pools), 96 beams (the dense phase 1), the early split
(one agent, four envs per workgroup) and the traffic early split (one ego, 32 NPC slots).
The poses come from tests/edge_poses.py (its first four kinds).  Each shape also states the rows
of the kernel tables its handle runs (Handle.step_row(): k_step's, k_serve's): a host-mode step
of a handle whose plan the persistent server holds (8x64_two_waves, 1x64_traffic_split) is
answered by that k_serve row whenever the server takes it, not launched; tests/test_edge_rows_gpu.py steps every k_step row
launched and every k_serve row served."""
import numpy as np
import pytest

import golden_replay as G
from conftest import STEP_KERNELS, use_step_kernel
from edge_poses import beam_quadrants, poses
import oracle_replay as ORP

pytestmark = pytest.mark.gpu

E, ROUNDS, RW, CR = 64, 3, 126.0, 84.0  # three lanes: the road's half width, the corner radius
SHAPES = [
    # rows: (k_step's row, k_serve's row) with the fused kernel asked for (kStepKeys, kServeKeys in csrc/mev_plan.h);
    # the default obs_dim makes plain rows of 31 + R floats, so 8 x 64 / 128 in one wave run the WC = 1 kernels
    dict(name="8x64_one_wave", n=8, rays=64, split=1, rows=(33, -1)),
    dict(name="8x64_two_waves", n=8, rays=64, rows=(16, 3)),
    dict(name="8x128_two_pools", n=8, rays=128, split=1, rows=(34, -1)),
    dict(name="8x96_dense", n=8, rays=96, split=1, rows=(26, -1)),
    dict(name="1x64_early_split", n=1, rays=64, pack=4, rows=(6, -1)),
    dict(name="1x64_traffic_split", n=1, rays=64, traffic=True, rows=(0, 0)),
]


def oracle_obs(shape, st, e, D):
    n = shape["n"]
    o = ORP.O.OracleEnv(num_lanes=3, n_agents=n, rays=shape["rays"], obs_dim=D, respawn=False,
                        traffic=bool(shape.get("traffic")), max_npcs=32)
    cars = ORP.O.new_cars(n)
    for a, b in ORP.EGO_FIELDS.items():
        cars[a] = st[b][e]
    o.set_state(cars, ORP.O.new_cars(0), int(st["step_count"][e]))
    r = o.step(np.zeros((n, 2), np.float32), 1.0 / 60.0, -1)
    o.close()
    return r["obs"]


def check_batch(shape, got, st, D):
    """Every env's observation against the oracle's; returns (beams that stopped, the set of
    direction quadrants in which a beam of an edge pose stopped)."""
    R_ = shape["rays"]
    for e in range(E):
        want = oracle_obs(shape, st, e, D)
        if not G.bits_equal(got[e], want):
            bad = np.argwhere(got[e].view(np.uint32) != want.view(np.uint32))
            i, c = bad[0]
            raise AssertionError(
                f"{shape['name']} env {e}: {len(bad)} words differ, first agent {i} col {c}: got {got[e][i, c]!r} "
                f"want {want[i, c]!r}; poses "
                f"{[(float(st['x'][e, j]), float(st['y'][e, j]), float(st['heading'][e, j])) for j in range(shape['n'])]}; "
                f"differing (agent, col): {bad[:12].tolist()}")
    lid = got[:, :, 31:31 + R_]
    stopped = (lid > 0) & (lid < 1.0)
    quad = beam_quadrants(st["heading"], R_)
    edge = stopped[0::4]  # the edge poses' envs
    return int(stopped.sum()), {q for q in range(4) if (edge & (quad[0::4] == q)).any()}


@pytest.mark.parametrize("kernel", STEP_KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s["name"] for s in SHAPES])
def test_lidar_matches_oracle_at_the_road_bounds_edges(mev, shape, kernel):
    rng = np.random.default_rng(20 + SHAPES.index(shape))
    n, R_ = shape["n"], shape["rays"]
    cfg = dict(traffic_flow=1, traffic_density=0.5, max_npcs=32) if shape.get("traffic") else {}
    h = mev.Handle(num_envs=E, num_agents=n, lidar_rays=R_, respawn_enabled=0, **cfg)
    use_step_kernel(mev, h, kernel)
    if kernel == 2:
        if "split" in shape:
            h.set_step_split(shape["split"])
        if "pack" in shape:
            h.set_step_pack(shape["pack"])
        want_split = 2 if ("pack" in shape or shape.get("traffic")) else (0 if shape.get("split") == 1 else 1)
        assert h.step_kernel() == 2 and h.step_split() == want_split, (h.step_kernel(), h.step_split())
        assert h.step_row() == dict(step=shape["rows"][0], serve=shape["rows"][1], tab=0), h.step_row()
    else:
        assert h.step_row() == dict(step=-1, serve=-1, tab=0), h.step_row()
    D = h.D
    stops, quads = 0, set()
    for _ in range(ROUNDS):
        st = h.get_state()
        st["x"][:], st["y"][:], st["heading"][:] = poses(rng, n)
        st["alive"][:] = 1
        for f in ("v", "acc", "steering"):
            st[f][:] = 0.0
        h.set_state(st)
        st = h.get_state()
        kw = dict(spawn_route=np.full(E, -1, np.int32)) if shape.get("traffic") else {}
        got = h.step(np.zeros((E, n, 2), np.float32), **kw)["obs"]
        s, q = check_batch(shape, got, st, D)
        stops += s
        quads |= q
    h.close()
    # the comparison is not vacuous: beams stopped, and from the edge poses in every direction quadrant
    assert stops > 0
    assert quads == {0, 1, 2, 3}, quads
