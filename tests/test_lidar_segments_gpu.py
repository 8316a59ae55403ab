"""The LiDAR car phase of the 8-slot fused kernels (lidar_body's segments by lane: lane
8 j + o is the segment of compacted alive agent j and box o) against the C restatement.

The method is test_lidar_stress_gpu.py's: plant cars with zero speed, take one zero-action
step with respawn off, compare that step's observations bit for bit with
oracle/marl_oracle.c.  Shapes: 64 envs of 8, 5 or 2 agents (2: several envs per wave, with
candidates only inside an env) x 64, 96 or 128 beams of the default world, so the rows with
the world at compile time are reached too; one wave per env (set_step_split(1)), a car and
a LiDAR wave (2) and the early split (3) wherever the plan takes it.

Planted env kinds (e % 4):
  0  a tight cluster (sigma 35 px) of overlapping boxes: "every beam" segments, several
     lookup passes of 3c, segments that run across pass boundaries;
  1  the cars on a ring of radius 120 px round the centre: every (agent, box) segment exists;
  2  two groups at opposite arm ends, 550 px apart, the second of one car: an agent with no
     candidate at all; in every second such env only one agent is alive, which skips the
     car phase;
  3  a pixel-aligned chain of touching boxes.
In half of the envs about a quarter of the agents are dead (a dead car is still a box), so
the pool has fewer alive agents than slots and the compacted index differs from the slot.

So that the comparison is not vacuous, every case checks that some beam of a sample of 8
envs is shorter than the same beam of an oracle run of that car alone, and that some LiDAR
pool holds at least 129 (beam, box) pairs by a host-side count from the planted boxes: a
lower bound (whole beam steps inside a box's angular span; every beam from inside a box).
The count is per pool because the pool is what 3c packs into lanes: at 8 agents x 96 or
128 beams an env is two pools, and two agents make at most 2 x 64 pairs per env, so there
the pool is the wave's envs."""
import zlib

import numpy as np
import pytest

import golden_replay as G
import oracle_replay as ORP

OracleEnv = ORP.O.OracleEnv

pytestmark = pytest.mark.gpu

E = 64
MAXD, STEP, FOV = 250.0, 4.0, 360.0  # the default world's LiDAR
EGO = {"x": "x", "y": "y", "v": "v", "h": "heading", "acc": "acc", "steer": "steering", "sx": "spawn_x",
       "sy": "spawn_y", "sv": "spawn_v", "sh": "spawn_heading", "prev_dist": "prev_dist", "pa0": "prev_a0",
       "pa1": "prev_a1", "path_index": "path_index", "route": "route", "intention": "intention", "alive": "alive"}


def plant(n, rays):
    """x, y, heading [E][n] float64 and alive [E][n] bool of the planted envs."""
    rng = np.random.default_rng(zlib.crc32(f"segments n{n} r{rays}".encode()))
    x, y, hd = np.zeros((E, n)), np.zeros((E, n)), np.zeros((E, n))
    alive = np.ones((E, n), bool)
    for e in range(E):
        kind = e % 4
        h = rng.uniform(-np.pi, np.pi, n)
        axis = rng.uniform(size=n) < 0.3  # axis-aligned headings (rays parallel to box edges)
        h[axis] = rng.integers(-2, 3, axis.sum()) * (np.pi / 2)
        if kind == 0:
            c = rng.uniform(150, 600, 2)
            xy = c + rng.normal(0, 35, (n, 2))
        elif kind == 1:
            a = rng.uniform(-np.pi, np.pi) + np.arange(n) * (2 * np.pi / n)
            r = 120.0 + rng.uniform(-3, 3, n)
            xy = np.stack([375 + r * np.cos(a), 375 - r * np.sin(a)], 1)
        elif kind == 2:
            far = rng.integers(0, 2)  # along which road the two arm ends lie
            t = np.where(np.arange(n) < n - 1, 100.0, 650.0) + rng.normal(0, 12, n)
            s = 375 + rng.normal(0, 30, n)
            xy = np.stack([t, s], 1) if far else np.stack([s, t], 1)
        else:
            t = np.arange(n) * rng.choice([24.0, 27.0, 54.0]) + rng.uniform(0, 1)
            ang = rng.uniform(-np.pi, np.pi)
            xy = np.stack([375 + np.cos(ang) * (t - t.mean()), 375 - np.sin(ang) * (t - t.mean())], 1)
            m = rng.uniform(size=n) < 0.5
            xy[m] = np.round(xy[m])
        x[e], y[e], hd[e] = xy[:, 0], xy[:, 1], h
        if (e // 4) % 2 == 1:
            alive[e] = rng.uniform(size=n) > 0.25
        if kind == 2 and (e // 8) % 2 == 1:
            alive[e] = np.arange(n) == rng.integers(0, n)
    return x, y, hd, alive


def host_pairs(x, y, hd, alive, rays):
    """A lower bound of the (beam, box) pairs of each viewer [E][n]: every car of the env but
    the viewer is a box (54 x 24 px, its pixel AABB) when within max_dist + 2 px; the viewer
    inside the box widened by the slab's margin sees it on every beam, else on at least one
    beam per whole beam step of the box's angular span."""
    n = x.shape[1]
    dphi = 2 * np.pi / (rays - 1)  # no smaller step spreads `rays` beams over 360 degrees
    out = np.zeros((E, n), np.int64)
    for e in range(E):
        ex = np.abs(np.cos(hd[e])) * 27.0 + np.abs(np.sin(hd[e])) * 12.0
        ey = np.abs(np.sin(hd[e])) * 27.0 + np.abs(np.cos(hd[e])) * 12.0
        x0, x1 = np.ceil(x[e] - ex), np.floor(x[e] + ex)
        y0, y1 = np.ceil(y[e] - ey), np.floor(y[e] + ey)
        for a in range(n):
            if not alive[e, a]:
                continue
            cx, cy = x[e, a], y[e, a]
            for o in range(n):
                if o == a:
                    continue
                ddx, ddy = max(x0[o] - cx, cx - x1[o], 0.0), max(y0[o] - cy, cy - y1[o], 0.0)
                if ddx * ddx + ddy * ddy > (MAXD + 1.0) ** 2:
                    continue
                if x0[o] <= cx <= x1[o] + 1 and y0[o] <= cy <= y1[o] + 1:
                    out[e, a] += rays
                    continue
                ang = np.array([np.arctan2(-(Y - cy), X - cx) for X in (x0[o], x1[o] + 1) for Y in (y0[o], y1[o] + 1)])
                ctr = np.arctan2(-(0.5 * (y0[o] + y1[o] + 1) - cy), 0.5 * (x0[o] + x1[o] + 1) - cx)
                d = (ang - ctr + np.pi) % (2 * np.pi) - np.pi
                out[e, a] += min(rays, max(0, int(np.floor((d.max() - d.min() - 1e-3) / dphi))))
    return out


def pool_slots(n, rays, pack, esplit):
    """Agent slots per LiDAR pool of a wave of `pack` envs (mev_layout.h step_pool_n, mev_step_body.inc)."""
    slots = pack * n
    if esplit:
        return slots
    if pack > 1:
        return min(max(512 // rays, 1), slots)
    g = max(512 // rays, 1)
    if g >= n:
        return n
    pools = -(-n // g)
    return -(-n // pools)


def oracle_step(n, rays, cars):
    o = OracleEnv(num_lanes=3, n_agents=n, rays=rays, fov=FOV, max_dist=MAXD, step=STEP, obs_dim=31 + rays,
                  respawn=False)
    o.set_state(cars, ORP.O.new_cars(0), 0)
    r = o.step(np.zeros((n, 2), np.float32))
    o.close()
    return r["obs"]


_REF = {}


def reference(h, n, rays):
    """The planted state of shape (n, rays) and the oracle's observations of its step, computed
    once and shared by the shape's split modes (every handle of a shape starts from the same state)."""
    if (n, rays) not in _REF:
        x, y, hd, alive = plant(n, rays)
        st = h.get_state()
        st["x"][:], st["y"][:], st["heading"][:] = x, y, hd
        st["alive"][:] = alive.astype(st["alive"].dtype)
        st["v"][:], st["acc"][:], st["steering"][:] = 0.0, 0.0, 0.0
        st["step_count"][:] = 0
        want, shorter = [], 0
        for e in range(E):
            cars = ORP.O.new_cars(n)
            for a, b in EGO.items():
                cars[a] = st[b][e]
            want.append(oracle_step(n, rays, cars))
            if e < 8 and alive[e].any():  # two envs of each kind: the first alive car's beams against its own alone
                i = int(np.argmax(alive[e]))
                alone = oracle_step(1, rays, cars[i:i + 1])
                shorter += int((want[e][i, 31:] < alone[0, 31:]).sum())
        _REF[(n, rays)] = (st, np.stack(want), shorter, host_pairs(x, y, hd, alive, rays))
    return _REF[(n, rays)]


def _cases():
    out = []
    for n in (8, 5, 2):
        for rays in (64, 96, 128):
            for mode in (1, 2, 3):
                # envs per wave: two-agent envs share a wave (4 of them; the early split holds its
                # slots' beams in one 512-beam pool: 2 envs beyond 64 beams)
                pack = 1 if n > 2 else (2 if mode == 3 and rays > 64 else 4)
                if mode == 3 and pack * n * rays > 512:
                    continue  # the plan has no early split for this shape
                out.append((n, rays, mode, pack))
    return out


@pytest.mark.parametrize("n,rays,mode,pack", _cases(), ids=[f"n{n}_r{r}_split{m}" for n, r, m, _ in _cases()])
def test_car_phase_matches_oracle(mev, n, rays, mode, pack):
    h = mev.Handle(num_envs=E, num_agents=n, lidar_rays=rays, respawn_enabled=0)
    try:
        h.set_step_kernel(2)
        h.set_step_pack(pack)
        h.set_step_split(mode)
        assert h.step_kernel() == 2 and h.step_pack() == pack and h.step_split() == mode - 1, (
            h.step_kernel(), h.step_pack(), h.step_split())
        st, want, shorter, pairs = reference(h, n, rays)
        h.set_state(st)
        got = h.step(np.zeros((E, n, 2), np.float32))["obs"]
        g = pool_slots(n, rays, pack, mode == 3)
        per_wave = pairs.reshape(E // pack, pack * n)
        pool_pairs = max(int(per_wave[:, j0:j0 + g].sum(1).max()) for j0 in range(0, pack * n, g))
        print(f"n {n} rays {rays} split {mode} pack {pack}: pool of {g} slots, most pairs in a pool >= {pool_pairs}, "
              f"sampled beams shortened by a car {shorter}")
        for e in range(E):
            if not G.bits_equal(got[e], want[e]):
                bad = np.argwhere(got[e].view(np.uint32) != want[e].view(np.uint32))
                i, c = bad[0]
                raise AssertionError(
                    f"env {e} (kind {e % 4}): {len(bad)} words differ, first agent {i} col {c}: got {got[e][i, c]!r} "
                    f"want {want[e][i, c]!r}; alive {st['alive'][e].tolist()}; differing (agent, col): {bad[:12].tolist()}")
        assert shorter > 0, "no sampled beam stops at a car"
        assert pool_pairs >= 129, f"no pool with more than two 64-pair chunks: {pool_pairs}"
    finally:
        h.close()
