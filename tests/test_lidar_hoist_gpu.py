"""LiDAR phase 1's agent pre-pass (lidar_body, csrc/mev_kernels.hip: the pass's pose by readlane, the
car centre's road region and on-screen test as wave-uniform bits) and the per-handle beam model
(csrc/mev_beams.h) in the one-wave k_step kernels, against the C oracle (oracle/marl_oracle.c): every
output of every step and the whole state after it, bit for bit.

Each case plants poses with set_state (zero speed, respawn off).  The first step has zero actions: with
zero throttle and zero speed Car::update leaves x and y as they are, bit for bit, so that step's LiDAR
starts from the planted centres (asserted on the state after it); the following steps have random
actions.  With respawn off a crashed ego keeps its alive flag, so the compacted agent index of the
pre-pass differs from the slot only through the agents planted dead (envs 4-6).  Planted, per env in turn:
  0, 7 car centres on each region border |p - 375| = rwm and one float32 step of the coordinate either
     side, on both axes and both signs (asserted from get_state before the step: all twelve are there);
  1 on a corner fillet (the general form) and in the centre cross;
  2 off screen on each of the four sides (no safe stretch: the march starts at probe 0);
  3 |heading| >= 100.  Car::update wraps the heading into [-pi, pi] (fmodf, unconditionally) before the
     step's LiDAR reads it, so these reach phase 1 wrapped and take the branch-free sincosf like any
     other: phase 1's `small = false` instantiation cannot be reached through mev_step with a finite
     heading, and no test here runs it (a NaN heading would, but the reference's own (int) of a NaN
     probe coordinate is undefined, so there is nothing to compare with).  The planted values check the
     wrap itself against the oracle;
  4 dead agents among the living (odd and even counts of alive agents);
  5 one alive agent (8 x 128: also a pool with none);
  6 no alive agent in the first pool / in the env.
"""
import os

import numpy as np
import pytest

import oracle_replay as ORP

pytestmark = pytest.mark.gpu

RW = 126.0  # three lanes: the road's half width
RWM = np.float32(RW - 1.5)  # the regions' border (mev_roadbound.h)
E, T = 16, 6


def _handle(mev, n, rays, no_world_const=False, split_off=True, **cfg):
    old = os.environ.pop("MEV_NO_WORLD_CONST", None)
    if no_world_const:
        os.environ["MEV_NO_WORLD_CONST"] = "1"  # read per handle at mev_create
    try:
        h = mev.Handle(num_envs=E, num_agents=n, lidar_rays=rays, respawn_enabled=0, seed=23, **cfg)
    finally:
        os.environ.pop("MEV_NO_WORLD_CONST", None)
        if old is not None:
            os.environ["MEV_NO_WORLD_CONST"] = old
    if split_off:
        h.set_step_split(1)  # one wave per env, as at 4096 envs
        assert h.step_kernel() == 2 and h.step_split() == 0 and h.step_pack() == 1
    return h


def _ulps(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-1e9)), v, np.nextafter(v, np.float32(1e9))]


def _border_coords():
    """(axis, coordinate): 375 -+ rwm and the float32 neighbours of that coordinate, per axis.  (p - 375 is
    exact for these, so |p - 375| is rwm and rwm -+ one step of the coordinate's own spacing: the region
    comparison |p - 375| < rwm is true on one side and false on the border and beyond.)"""
    c = np.float32(375.0)
    return [(axis, b) for axis in (0, 1) for s in (-1.0, 1.0) for b in _ulps(c + np.float32(s) * RWM)]


def _plant(rng, st, n):
    x, y, hd, alive = st["x"], st["y"], st["heading"], st["alive"]
    border, slot = _border_coords(), 0
    for e in range(E):
        k = e % 8
        arm = rng.integers(0, 2, n).astype(bool)
        along = rng.choice([-1.0, 1.0], n) * rng.uniform(RW + 20.0, 360.0, n)
        across = rng.uniform(-(RW - 15.0), RW - 15.0, n)
        x[e] = 375.0 + np.where(arm, along, across)
        y[e] = 375.0 + np.where(arm, across, along)
        hd[e] = rng.uniform(-np.pi, np.pi, n)
        alive[e] = 1
        if k in (0, 7):
            for i in range(n):
                axis, b = border[slot % len(border)]
                slot += 1
                if axis == 0:
                    x[e, i] = b
                else:
                    y[e, i] = b
        elif k == 1:
            sg = rng.choice([-1.0, 1.0], (2, n))
            x[e] = 375.0 + sg[0] * rng.uniform(RW - 1.5, RW + 12.0, n)
            y[e] = 375.0 + sg[1] * rng.uniform(RW - 1.5, RW + 12.0, n)
            x[e, 0], y[e, 0] = 375.0 + rng.uniform(-60, 60), 375.0 + rng.uniform(-60, 60)
        elif k == 2:
            off = [(-3.5, 375.0), (752.25, 380.0), (370.0, -0.75), (381.0, 750.0), (-40.0, 800.0), (749.9995, 749.9995)]
            for i in range(n):
                x[e, i], y[e, i] = off[(i + e // 8) % len(off)]
        elif k == 3:
            hd[e, 0] = 100.0
            hd[e, n - 1] = -(100.0 + rng.uniform(0.0, 400.0))
            if n > 4:
                hd[e, 4] = 250.0
        elif k == 4:
            alive[e, 0] = 0
            if n > 3:
                alive[e, 2] = 0
            if n > 5 and e >= 8:
                alive[e, 5] = 0
        elif k == 5:
            alive[e] = 0
            alive[e, n - 2] = 1
        elif k == 6:
            alive[e] = 0
            if e >= 8 and n > 4:
                alive[e, 4:] = 1  # (8 x 128: the first pool empty, the second full)
    for f in ("v", "acc", "steering"):
        st[f][:] = 0.0


def _oracle(h, n, rays, st, e, rel=None):
    o = ORP.O.OracleEnv(num_lanes=3, n_agents=n, rays=rays, obs_dim=h.D, respawn=False)
    if rel is not None:
        o.set_rel_angles(rel)
    cars = ORP.O.new_cars(n)
    for a, b in ORP.EGO_FIELDS.items():
        cars[a] = st[b][e]
    o.set_state(cars, ORP.O.new_cars(0), int(st["step_count"][e]))
    return o


def _drive(h, n, rays, tag, rel=None, steps=T, plant=True):
    """Plant, then `steps` steps against one oracle per env; returns (beams that stopped, alive counts seen)."""
    rng = np.random.default_rng(100 * n + rays)
    st = h.get_state()
    if plant:
        _plant(rng, st, n)
        h.set_state(st)
    st = h.get_state()
    if plant and 4 * n >= 12:  # (envs 0, 7, 8, 15: 4 n border slots)
        c = np.float32(375.0)
        for axis, b in _border_coords():
            assert (st["xy"[axis]][0::8] == b).any() or (st["xy"[axis]][7::8] == b).any(), (tag, axis, float(b))
        for f in ("x", "y"):  # one side inside, the border itself and the far side outside, both signs
            r = st[f].astype(np.float32) - c
            for sg in (-1.0, 1.0):
                d = np.abs(r[np.sign(r) == sg]) - RWM
                assert (d == 0).any() and ((d < 0) & (d > -1e-4)).any() and ((d > 0) & (d < 1e-4)).any(), (tag, f, sg)
    oracles = [_oracle(h, n, rays, st, e, rel) for e in range(E)]
    stops, counts, shifted = 0, set(), False
    try:
        for t in range(steps):
            alive = h.get_state()["alive"] != 0
            counts |= {int(c) for c in alive.sum(axis=1)}
            # a compacted index that differs from the slot: a dead agent below an alive one
            shifted |= bool((~alive[:, :-1] & alive[:, 1:]).any())
            a = rng.uniform(-1, 1, (E, n, 2)).astype(np.float32)
            a[..., 0] = rng.uniform(0.5, 1.0, (E, n)).astype(np.float32)
            if t == 0:
                a[:] = 0.0  # the planted centres are the ones this step's LiDAR starts from
            out = {k: np.array(v) for k, v in h.step(a).items()}
            gst = h.get_state()
            if t == 0:
                for f in ("x", "y"):
                    assert np.array_equal(gst[f].view(np.uint32), st[f].view(np.uint32)), (tag, f, "moved")
            for e in range(E):
                r = oracles[e].step(a[e], 1.0 / 60.0, -1)
                ORP.check_step(f"{tag} step {t + 1} env {e}", out, e, r)
                ORP.check_state(f"{tag} step {t + 1} env {e}", gst, e, oracles[e])
            lid = out["obs"][:, :, 31:31 + rays]
            stops += int(((lid > 0) & (lid < 1.0)).sum())
    finally:
        for o in oracles:
            o.close()
    assert stops > 0 and shifted, (tag, stops, shifted)
    return stops, counts


@pytest.mark.parametrize("no_wc", [False, True], ids=["world-const", "world-runtime"])
@pytest.mark.parametrize("rays", [64, 128])
def test_eight_agents_match_the_oracle(mev, rays, no_wc):
    h = _handle(mev, 8, rays, no_world_const=no_wc)
    try:
        _, counts = _drive(h, 8, rays, f"8x{rays}")
    finally:
        h.close()
    assert {0, 1}.issubset(counts) and any(c % 2 for c in counts if c > 1), counts  # none, one, an odd count


@pytest.mark.parametrize("n", [5, 3])
def test_odd_agent_counts_match_the_oracle(mev, n):
    h = _handle(mev, n, 64)
    try:
        _, counts = _drive(h, n, 64, f"{n}x64")
    finally:
        h.close()
    assert n in counts, counts  # the last pass repeats an agent


def test_served_host_steps_match_the_oracle(mev):
    """A host-mode handle of 8 x 64 beams with the split left to the plan: the persistent server (k_serve)
    answers its steps -- the early split's LiDAR wave, which reads the beam model too."""
    h = _handle(mev, 8, 64, split_off=False)
    try:
        assert h.step_row()["serve"] >= 0, h.step_row()
        _drive(h, 8, 64, "served 8x64")
        assert h.serve_stats()["steps"] == T, h.serve_stats()
    finally:
        h.close()


@pytest.mark.parametrize("rays", [64, 128])
def test_rewritten_beam_list_is_followed(mev, rays):
    """mev_set_beam_angles after creation: the cached model follows the new offsets (a 120 degree fan, then
    the same fan reversed, which has no linear model: every beam against every box)."""
    h = _handle(mev, 8, rays)
    try:
        fan = (np.linspace(-60.0, 60.0, rays, dtype=np.float64) * np.pi / 180.0).astype(np.float32)
        h.set_beam_angles(fan)
        assert np.array_equal(h.beam_angles(), fan)
        _drive(h, 8, rays, f"fan 8x{rays}", rel=fan, steps=3)
        h.set_beam_angles(fan[::-1].copy())
        _drive(h, 8, rays, f"reversed fan 8x{rays}", rel=fan[::-1].copy(), steps=2)
    finally:
        h.close()
