"""Poses at which a LiDAR or status kernel can go wrong, for the tests that compare the device
with the C restatement (test_road_bound_gpu.py, test_edge_rows_gpu.py) and for the fixtures
recorded from the reference at the same poses (tests/golden/gen_golden.py group `edge`,
tests/golden/edge_<config>.npz, test_edge_fixtures.py).

Kinds, interleaved by env (env e holds kind e % kinds):
  0 grass    within 3 px of a grass edge, half of them on whole pixels
  1 disc     on the rims of the corner discs, +- 4 px
  2 centre   inside the centre square
  3 off      off the road / off the screen
  4 border   the centre within 1.5 px of 0 or 750 in x or y, on the road's strip; half of them in
             (-1, 0) and (749, 751): int() truncates toward zero, so a probe at -0.4 is pixel 0, on
             screen (Lidar.cpp:34-40), and one at 750.3 is pixel 750, off it
  5 box      pairs (observer 2k, target 2k + 1) on whole pixels with axis-aligned headings: the
             observer's beam 0 runs along an axis (dx or dy exactly +-1), and a probe pixel of it
             falls exactly on x +- ex / y +- ey of the target's box (the test is inclusive,
             Lidar.cpp:74-75) or on the pixel just outside it
  6 twins    pairs whose x, y and heading differ componentwise by 0, +-0.0009 or +-0.0011: cars
             closer than 1e-3 in all three do not see each other (Lidar.cpp:59-63)
The first four are the generator test_road_bound_gpu.py has used since the road bound; with
kinds=4 and three lanes the random stream and the poses are what they were."""
from __future__ import annotations

import json
import os

import numpy as np

KINDS = ("grass", "disc", "centre", "off", "border", "box", "twins")
EDGE_KINDS = (0, 1, 4)  # the kinds whose stopped beams must cover every direction quadrant
LANE_W, CR = 42.0, 84.0  # a lane's width, the corner radius
TWIN_DELTAS = (0.0, 0.0009, -0.0009, 0.0011, -0.0011)
# the arms of the cross: the outward direction (dx, dy) and the beam angle that has it (dx = cos, dy = -sin)
ARMS = ((1, 0, 0.0), (-1, 0, -np.pi), (0, 1, -np.pi / 2), (0, -1, np.pi / 2))


def probe_distances(max_dist=250.0, lidar_step=4.0):
    """The distances Lidar::update probes, accumulated in float32 (Lidar.cpp:33)."""
    out, d, st, mx = [], np.float32(0.0), np.float32(lidar_step), np.float32(max_dist)
    while d < mx:
        out.append(d)
        d = np.float32(d + st)
    return np.array(out, np.float32)


def poses(rng, n, E=64, num_lanes=3, kinds=4, fov=360.0, lidar_step=4.0, dims=None, npcs=0):
    """x, y, heading [E][n]; env e holds poses of kind e % kinds.  Agent i of an env takes quadrant
    i % 4 (and the far half of its edge for i >= 4), so few cars of an env overlap.  fov and
    lidar_step: the LiDAR's, dims: (length, width) per agent (default 54 x 24) -- the box kind places
    its targets by them.  npcs: the last `npcs` of the n cars are NPCs behind one ego (traffic): of
    the box and twin kinds only (the ego, NPC 0) pair up -- NPCs that overlap remove each other
    (TrafficFlow.cpp:346-362) -- and NPC 1 stands ahead of NPC 0 and beside it, so that NPC 0 brakes
    and keeps its pose through the step (get_front_car_dist_tf: closer than 50 px, within 37 degrees)."""
    RW = LANE_W * num_lanes
    probes = probe_distances(250.0, lidar_step)
    probes = probes[(probes >= 32) & (probes <= 80)]
    x, y = np.zeros((E, n)), np.zeros((E, n))
    ccen = RW + CR
    fixed_h = {}  # (e, i) -> heading of the kinds that set it
    for e in range(E):
        kind = e % kinds
        for i in range(n):
            j = i if n > 1 else int(rng.integers(0, 8))
            sx, sy = (1, -1)[j & 1], (1, -1)[(j >> 1) & 1]
            far = j >= 4
            paired = kind in (5, 6) and (i | 1) < (2 if npcs else n)  # (the others stand in the centre square)
            if kind == 0:
                u = RW + rng.uniform(-3, 3)  # the strip's edge; along it: from the corner square to the screen's edge
                v = rng.uniform(RW + 40, ccen + 40) if far else rng.uniform(ccen + 60, 370)
                if rng.uniform() < 0.3:  # the corner square's outer edge
                    u, v = rng.uniform(RW + 5, ccen - 5), ccen + rng.uniform(-3, 3)
                if rng.uniform() < 0.5:
                    u, v = v, u
            elif kind == 1:
                a, rad = rng.uniform(np.pi, 1.5 * np.pi), CR + rng.uniform(-4, 4)
                u, v = ccen + rad * np.cos(a), ccen + rad * np.sin(a)
            elif kind in (5, 6) and npcs and i == 2:  # NPC 0's blocker: 40 px ahead, 26 px beside, its heading
                hb = fixed_h[(e, i)] = fixed_h[(e, 1)]
                x[e, i] = x[e, 1] + 40 * np.cos(hb) + 26 * np.sin(hb)
                y[e, i] = y[e, 1] - 40 * np.sin(hb) + 26 * np.cos(hb)
                continue
            elif kind == 2 or (kind in (5, 6) and not paired):
                u, v = rng.uniform(0, ccen, 2)
            elif kind == 3:
                u, v = rng.uniform(RW + 10, 400, 2) if far else (rng.uniform(0, RW), rng.uniform(365, 400))
            elif kind == 4:
                side = 750.0 * ((j >> 1) & 1)
                c = side + rng.uniform(-1.5, 1.5)
                if rng.uniform() < 0.5:
                    c = rng.uniform(-1.0, 0.0) if side == 0 else rng.uniform(749.0, 751.0)
                lat = 375.0 + rng.uniform(-(RW - 15), RW - 15)
                x[e, i], y[e, i] = (c, lat) if j & 1 else (lat, c)
                continue
            elif kind == 5:
                ax, ay, ang = ARMS[(i // 2 + e // kinds) % 4]  # (every arm in turn, also with one pair per env)
                if i % 2 == 0:  # the observer: on whole pixels, beam 0 (heading - fov / 2) outward along the arm
                    t = int(rng.integers(40, 121))
                    lat = int(rng.integers(-(int(RW) - 40), int(RW) - 39))
                    x[e, i], y[e, i] = 375 + ax * t + ay * lat, 375 + ay * t + ax * lat
                    fixed_h[(e, i)] = (ang + np.radians(fov) / 2 + np.pi) % (2 * np.pi) - np.pi
                else:  # the target (heading 0): its near face on a probe's pixel, or one pixel further out
                    ln, wd = (54.0, 24.0) if dims is None else dims[i % len(dims)]
                    pd, s = rng.choice(probes), int(rng.integers(0, 2))
                    # (the probe's pixel: int() of the observer's whole pixel +- the distance, in float32)
                    c0 = np.float32(x[e, i - 1] if ax else y[e, i - 1])
                    px = abs(int(np.float32(c0 + np.float32(ax + ay) * pd)) - int(c0))
                    d = px + (ln if ax else wd) / 2 + s
                    hl = int((wd if ax else ln) / 2)  # across the beam: on the box's side edge, one pixel in, one out
                    dl = int(rng.choice([-hl - 1, -hl, -hl + 1, 0, 0, hl - 1, hl, hl + 1]))
                    x[e, i], y[e, i] = x[e, i - 1] + ax * d + ay * dl, y[e, i - 1] + ay * d + ax * dl
                    fixed_h[(e, i)] = 0.0
                continue
            else:  # twins
                if i % 2 == 0:
                    ax, ay, _ = ARMS[(i // 2 + e // kinds) % 4]
                    t, lat = rng.uniform(100, 300), rng.uniform(-(RW - 30), RW - 30)
                    x[e, i], y[e, i] = 375 + ax * t + ay * lat, 375 + ay * t + ax * lat
                    fixed_h[(e, i)] = rng.uniform(-3.0, 3.0)
                else:
                    dx, dy, dh = rng.choice(TWIN_DELTAS, 3)
                    # (in float32, as the state holds them: the twin is the first car's value plus delta)
                    x[e, i] = float(np.float32(x[e, i - 1])) + dx
                    y[e, i] = float(np.float32(y[e, i - 1])) + dy
                    fixed_h[(e, i)] = float(np.float32(fixed_h[(e, i - 1)])) + dh
                continue
            x[e, i], y[e, i] = 375 + sx * u, 375 + sy * v
            if kind == 0 and rng.uniform() < 0.5:
                x[e, i], y[e, i] = np.round(x[e, i]), np.round(y[e, i])
    h = rng.uniform(-np.pi, np.pi, (E, n))
    axis = rng.uniform(size=(E, n)) < 0.4
    h[axis] = rng.integers(-2, 3, int(axis.sum())) * (np.pi / 2)
    for (e, i), v in fixed_h.items():
        h[e, i] = v
    return x, y, h


def beam_quadrants(h, rays, fov=360.0):
    """[..., rays] the direction quadrant (0..3 by the signs of dx, dy) of every beam of a car with
    heading h, -1 within 0.01 rad of an axis (Lidar.cpp:24-26: dx = cos, dy = -sin of h + rel)."""
    rel = (-0.5 * fov + np.arange(rays) * (fov / (rays - 1))) * (np.pi / 180.0)
    ang = np.asarray(h, np.float64)[..., None] + rel
    dx, dy = np.cos(ang), -np.sin(ang)
    q = (dx < 0).astype(int) + 2 * (dy < 0).astype(int)
    return np.where((np.abs(dx) < 0.01) | (np.abs(dy) < 0.01), -1, q)


# ---- the fixtures recorded from the reference (tests/golden/edge_<name>.npz) ----
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EGO_DIMS = [(80.0, 30.0), (40.0, 18.0), (54.0, 24.0), (70.0, 36.0), (30.0, 12.0), (110.0, 22.0), (60.0, 60.0),
            (20.0, 40.0)]
_BASE = dict(n=8, rays=64, lanes=3, fov=360.0, max_dist=250.0, lidar_step=4.0, dims=False, traffic=0, npcs=0)
# name -> configuration, pose sets P (a multiple of 16, >= 64) and seed.  Seeds are chosen so that
# the recorded reference data alone satisfies test_edge_fixtures.py's non-vacuity counts.
FIXTURES = {
    "n8_r64": dict(_BASE, P=64, seed=7001),
    "n8_r64_lanes2": dict(_BASE, lanes=2, P=64, seed=7002),
    "n12_r96_fov120_maxd180_step33": dict(_BASE, n=12, rays=96, fov=120.0, max_dist=180.0, lidar_step=3.3, P=64,
                                          seed=7003),
    "n8_r128_dims": dict(_BASE, rays=128, dims=True, P=64, seed=7004),
    "traffic_n1_k7": dict(_BASE, n=1, traffic=1, npcs=7, P=256, seed=7006),
}
CONFIG_KEYS = ("n", "rays", "lanes", "fov", "max_dist", "lidar_step", "dims", "traffic")


def fixture_names():
    return list(FIXTURES)


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN_DIR, f"edge_{name}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def fixture_for(cfg):
    """The fixture whose configuration equals cfg's in CONFIG_KEYS (a traffic fixture needs its NPC
    slots, too), or None."""
    for name, f in FIXTURES.items():
        if all(cfg[k] == f[k] for k in CONFIG_KEYS) and cfg.get("max_npcs", 32) >= f["npcs"]:
            return name
    return None
