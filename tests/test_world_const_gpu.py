"""The k_step instantiations that hold the reference's world and the plain row layout at
compile time (StepKey::wc, csrc/mev_refworld.h) against the kernels that read them at run
time: two handles of the same configuration, one created under MEV_NO_WORLD_CONST=1, stepped
with the same seeded actions -- every output of every step and the whole state every 20
steps, bit for bit.  64 envs with the split off run the one-wave-per-env kernel that 4096
envs run (the metric's instantiation at 64 beams, config 5's at 128).  Handles with another
world or another row layout must not take the specialised kernel: the same comparison
catches a folded constant applied to them."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, N, T, MAX_STEPS = 64, 8, 200, 40


def _handle(mev, no_world_const, **cfg):
    old = os.environ.pop("MEV_NO_WORLD_CONST", None)
    if no_world_const:
        os.environ["MEV_NO_WORLD_CONST"] = "1"  # read per handle at mev_create
    try:
        h = mev.Handle(num_envs=E, num_agents=N, use_team_reward=1, respawn_enabled=1, max_steps=MAX_STEPS, seed=11,
                       device=0, **cfg)
    finally:
        os.environ.pop("MEV_NO_WORLD_CONST", None)
        if old is not None:
            os.environ["MEV_NO_WORLD_CONST"] = old
    h.set_step_split(1)  # one wave per env, as at 4096 envs
    assert h.step_kernel() == 2 and h.step_split() == 0 and h.step_pack() == 1
    return h


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run_pair(mev, **cfg):
    """Step a default handle and a MEV_NO_WORLD_CONST=1 handle of configuration cfg together;
    returns how many env truncations, auto-resets and in-step respawns the run contained."""
    ha, hb = _handle(mev, False, **cfg), _handle(mev, True, **cfg)
    rng = np.random.default_rng(5)
    trunc = resets = respawns = 0
    ended = np.zeros(E, bool)
    try:
        for k, v in ha.get_state().items():
            assert np.array_equal(_bits(v), _bits(hb.get_state()[k])), k
        for t in range(T):
            a = rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)
            a[..., 0] = rng.uniform(0.5, 1.0, (E, N)).astype(np.float32)  # throttle: the cars get somewhere
            oa = {k: np.array(v) for k, v in ha.step(a, auto_reset=True).items()}
            ob = hb.step(a, auto_reset=True)
            assert set(oa) == set(ob)
            for k in oa:
                assert np.array_equal(_bits(oa[k]), _bits(ob[k])), (t, k)
            if (t + 1) % 20 == 0:
                sa, sb = ha.get_state(), hb.get_state()
                assert set(sa) == set(sb)
                for k in sa:
                    assert np.array_equal(_bits(sa[k]), _bits(sb[k])), (t, k)
            now = (oa["terminated"] != 0) | (oa["truncated"] != 0)
            trunc += int((oa["truncated"] != 0).sum())
            resets += int((ended & (oa["step"] == 1)).sum())
            respawns += int(((oa["done"] != 0) & (oa["status"] >= 2) & ~now[:, None]).sum())
            ended = now
    finally:
        ha.close()
        hb.close()
    return trunc, resets, respawns


@pytest.mark.parametrize("rays", [64, 128])
def test_world_const_kernel_equals_the_runtime_kernel(mev, rays):
    trunc, resets, respawns = _run_pair(mev, lidar_rays=rays)
    assert trunc >= E and resets >= E and respawns > 0, (trunc, resets, respawns)


@pytest.mark.parametrize("cfg", [dict(lidar_rays=64, num_lanes=2), dict(lidar_rays=64, obs_dim=127),
                                 dict(lidar_rays=64, lidar_max_dist=200.0)],
                         ids=["two-lanes", "obs-dim-127", "max-dist-200"])
def test_other_worlds_and_rows_keep_their_kernel(mev, cfg):
    trunc, resets, _ = _run_pair(mev, **cfg)
    assert trunc >= E and resets >= E, (trunc, resets)
