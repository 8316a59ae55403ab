"""Diagnostic: the LiDAR car phase's (phase 3) work per beam pool, segcnt build
(python tools/variants.py segcnt).
    python tools/seg_counts.py [--rays 64] [--envs 4096] [--agents 8]
Per pool of the fused k_step: segments M ((agent, candidate box) with the box within
range), pairs T ((beam, box) inside a box's angular span) and the lookup passes of 3c,
sampled every 7th step of a uniform-random-action rollout with resets, as the CPU
estimate that sized the car phase was."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pkgload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--steps", type=int, default=700)
    a = ap.parse_args()
    mev = pkgload.load()
    mev._capi.VARIANT = "segcnt"
    h = mev.Handle(num_envs=a.envs, num_agents=a.agents, lidar_rays=a.rays, use_team_reward=1, respawn_enabled=1,
                   max_steps=2000)  # (bench.py's handle)
    h.set_step_kernel(2)
    pools = 2 if a.agents * a.rays > 512 else 1
    rng = np.random.default_rng(0)
    rows = []
    for t in range(a.steps):
        h.step(rng.uniform(-1, 1, (a.envs, a.agents, 2)).astype(np.float32), auto_reset=True)
        if t % 7 == 6:
            d = h.debug_stamps().reshape(a.envs, 8).astype(np.int64)
            rows.append(np.concatenate([d[:, 3 * k:3 * k + 3] for k in range(pools)]))
    d = np.concatenate(rows)

    def stat(name, v):
        print(f"  {name:24s} mean {v.mean():7.2f}  p10 {np.percentile(v, 10):6.1f}  p50 {np.percentile(v, 50):6.1f}"
              f"  p90 {np.percentile(v, 90):6.1f}  max {v.max():6.1f}")

    print(f"{a.envs} envs x {a.agents} agents x {a.rays} beams, {pools} pool(s) per env, {len(rows)} sampled steps, "
          f"{len(d)} pools")
    stat("segments M", d[:, 0])
    stat("pairs T", d[:, 1])
    stat("3c passes", d[:, 2])
    stat("pairs / 64, rounded up", (d[:, 1] + 63) // 64)
    stat("pairs / 128, rounded up", (d[:, 1] + 127) // 128)
    print(f"  pools with no segment: {100.0 * (d[:, 0] == 0).mean():.1f} %")
    h.close()


if __name__ == "__main__":
    main()
