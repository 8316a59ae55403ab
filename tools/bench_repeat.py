"""What a frame-skip call (mev_step_repeat) saves over the same sub-steps as single steps.

Shapes: BASELINE config 3 (4096 envs x 8 agents x 64 beams, team reward) and config 4
(4096 x 1 x 64, traffic at density 0.5).  For repeat n in 1, 2, 4, 8: the time of 50
mev_step_repeat calls against the time of 50 * n mev_step calls on the same handle (the same
action tensor for the n steps of a window, device pointers, auto-reset), by stream events,
five times each, alternating -- after a clock settle and a warm-up as bench.py does.  The
single steps run the handle's automatic step kernel (what bench.py measures), the repeat calls
the looping car kernel plus one LiDAR cast.  Per shape also the two-kernel path's own split
(k_cars, with the NPC phase, against k_lidar: mev_kernel_timing), which says how much of a
step a repeat call can leave out at all.
    python tools/bench_repeat.py [--out profiles/repeat_sweep.json] [--only cfg3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [
    dict(name="cfg3", desc="4096 envs x 8 agents x 64 beams, team reward", E=4096, N=8, R=64, team=1),
    dict(name="cfg4", desc="4096 envs x 1 agent x 64 beams, traffic density 0.5", E=4096, N=1, R=64, traffic=1),
]
REPEATS = (1, 2, 4, 8)
CALLS, RUNS, WARMUP, SETTLE_MS = 50, 5, 100, 200.0


def measure(cfg):
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R = cfg["E"], cfg["N"], cfg["R"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, use_team_reward=cfg.get("team", 0),
                   traffic_flow=cfg.get("traffic", 0), traffic_density=0.5, max_steps=2000, seed=0, device=0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    h.set_stream(st.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    acts = torch.rand((CALLS, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
    rout = dict(out, substeps=torch.zeros(E, dtype=torch.int32, device=dev))
    h.reset(device=True)

    def single(c):
        h.step(acts[c].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)

    # clock settle, then warm-up (both untimed; traffic: the fleets build up meanwhile)
    n_settle = 0
    t_end = time.perf_counter() + SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            single(n_settle % CALLS)
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(WARMUP):
        single(t % CALLS)
    h.step_repeat(acts[0].data_ptr(), 2, 1.0 / 60.0, out=rout, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)
    fused = h.step_kernel() == 2

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    rows = []
    for n in REPEATS:
        def repeat_calls():
            for c in range(CALLS):
                h.step_repeat(acts[c].data_ptr(), n, 1.0 / 60.0, out=rout, auto_reset=True, device=True)

        def single_steps():
            for c in range(CALLS):
                for _ in range(n):
                    single(c)

        rep_ms, one_ms = [], []
        for _ in range(RUNS):
            one_ms.append(timed(single_steps) / CALLS)
            rep_ms.append(timed(repeat_calls) / CALLS)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        rows.append(dict(
            repeat=n,
            repeat_call_ms=round(med(rep_ms), 5), repeat_call_ms_min_max=[round(min(rep_ms), 5), round(max(rep_ms), 5)],
            single_steps_ms=round(med(one_ms), 5), single_steps_ms_min_max=[round(min(one_ms), 5), round(max(one_ms), 5)],
            repeat_agent_substeps_per_s=round(E * N * n / (med(rep_ms) * 1e-3), 1),
            single_agent_substeps_per_s=round(E * N * n / (med(one_ms) * 1e-3), 1),
            ratio_single_over_repeat=round(med(one_ms) / med(rep_ms), 4),
            gap_ms=round(med(one_ms) - med(rep_ms), 5),
            gap_exceeds_spread=bool(min(one_ms) - max(rep_ms) > max(max(rep_ms) - min(rep_ms), max(one_ms) - min(one_ms))),
            mean_substeps=round(float(rout["substeps"].float().mean()), 3)))
    # the two-kernel path's split (every 4th step: the events add their own launch latency)
    h.set_step_kernel(1)
    for t in range(20):
        single(t)
    torch.cuda.synchronize(dev)
    h.kernel_timing(4)
    for t in range(200):
        single(t % CALLS)
    torch.cuda.synchronize(dev)
    c_ms, l_ms, k = h.kernel_times()
    npc = float(h.get_state()["npc_count"].mean()) if cfg.get("traffic") else 0.0
    h.close()
    return dict(name=cfg["name"], workload=cfg["desc"], single_step_kernel="k_step (fused)" if fused else "k_cars + k_lidar",
                calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP,
                two_kernel_split_ms=dict(k_cars=round(c_ms / k, 5), k_lidar=round(l_ms / k, 5)),
                mean_npcs=round(npc, 2), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    res = dict(method="stream events around 50 mev_step_repeat calls / 50 * n mev_step calls, 5 runs each (median, "
                      "min-max), one process, one device; device pointers, auto-reset, the same actions for the n "
                      "steps of a window",
               device=torch.cuda.get_device_name(0), shapes=[])
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
