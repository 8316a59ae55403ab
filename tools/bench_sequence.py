"""What a plan rollout (mev_step_sequence) costs against what a planner pays without it.

Shapes: BASELINE config 3 (4096 envs x 8 agents x 64 beams, team reward) and config 4
(4096 x 1 x 64, traffic at density 0.5).  For a plan length T in 2, 4, 8, 16, the time of 50
calls, by stream events, five times each, alternating, after a clock settle and a warm-up as
bench.py does (device pointers, auto-reset, one session, one device):
  seq       mev_step_sequence with the three per-step arrays (reward_seq, done_seq, status_seq)
  seq_bare  mev_step_sequence without them
  single    (a) T mev_step calls with the same per-step actions on the same handle -- what a
            planner pays today (the handle's automatic step kernel, as bench.py measures)
  repeat    (b) mev_step_repeat(n = T), the held-action ceiling of the same kernel
Also, at config 3's shape, mev_restore_map against a masked mev_restore (the same grid).
MEV_LIB_VARIANT=seqearly (tools/variants.py) measures the build that issues a sub-step's action
load ahead of the previous sub-step's row stores.
    python tools/bench_sequence.py [--out profiles/sequence_sweep.json] [--only cfg3]"""
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
LENGTHS = (2, 4, 8, 16)
CALLS, RUNS, WARMUP, SETTLE_MS = 50, 5, 100, 200.0
PLANS = 8  # distinct plans cycled through the 50 calls


def med(v):
    return sorted(v)[len(v) // 2]


def stat(v):
    return dict(ms=round(med(v), 5), min_max=[round(min(v), 5), round(max(v), 5)], spread=round(max(v) - min(v), 5))


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
    tmax = max(LENGTHS)
    acts = torch.rand((PLANS, tmax, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
    rout = dict(out, substeps=torch.zeros(E, dtype=torch.int32, device=dev))
    h.reset(device=True)

    def single(ptr):
        h.step(ptr, 1.0 / 60.0, out=out, auto_reset=True, device=True)

    n_settle = 0
    t_end = time.perf_counter() + SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            single(acts[n_settle % PLANS, 0].data_ptr())
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(WARMUP):
        single(acts[t % PLANS, t % tmax].data_ptr())
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
    for T in LENGTHS:
        sout = dict(rout, reward_seq=torch.zeros((T, E, N), dtype=torch.float32, device=dev),
                    done_seq=torch.zeros((T, E, N), dtype=torch.uint8, device=dev),
                    status_seq=torch.zeros((T, E, N), dtype=torch.uint8, device=dev))

        def seq_calls():
            for c in range(CALLS):
                h.step_sequence(acts[c % PLANS].data_ptr(), 1.0 / 60.0, out=sout, auto_reset=True, device=True, length=T)

        def seq_bare_calls():
            for c in range(CALLS):
                h.step_sequence(acts[c % PLANS].data_ptr(), 1.0 / 60.0, out=rout, auto_reset=True, device=True, length=T)

        def repeat_calls():
            for c in range(CALLS):
                h.step_repeat(acts[c % PLANS, 0].data_ptr(), T, 1.0 / 60.0, out=rout, auto_reset=True, device=True)

        def single_steps():
            for c in range(CALLS):
                for s in range(T):
                    single(acts[c % PLANS, s].data_ptr())

        seq_calls()
        repeat_calls()
        torch.cuda.synchronize(dev)
        t_seq, t_bare, t_one, t_rep = [], [], [], []
        for _ in range(RUNS):
            t_one.append(timed(single_steps) / CALLS)
            t_rep.append(timed(repeat_calls) / CALLS)
            t_seq.append(timed(seq_calls) / CALLS)
            t_bare.append(timed(seq_bare_calls) / CALLS)
        seq_calls()
        torch.cuda.synchronize(dev)
        spread3 = 3.0 * max(max(v) - min(v) for v in (t_seq, t_bare, t_rep))
        rows.append(dict(
            length=T, seq=stat(t_seq), seq_bare=stat(t_bare), single_steps=stat(t_one), repeat=stat(t_rep),
            ratio_single_over_seq=round(med(t_one) / med(t_seq), 4),
            seq_agent_substeps_per_s=round(E * N * T / (med(t_seq) * 1e-3), 1),
            seq_minus_repeat_ms=round(med(t_seq) - med(t_rep), 5),
            seq_bare_minus_repeat_ms=round(med(t_bare) - med(t_rep), 5),
            three_run_spreads_ms=round(spread3, 5),
            seq_minus_repeat_exceeds_three_spreads=bool(med(t_seq) - med(t_rep) > spread3),
            mean_substeps=round(float(sout["substeps"].float().mean()), 3)))
    # us per further sub-step: the slope of the call time over the plan length
    for key in ("seq", "seq_bare", "repeat"):
        lo, hi = rows[0], rows[-1]
        slope = (hi[key]["ms"] - lo[key]["ms"]) / (hi["length"] - lo["length"]) * 1e3
        for r in rows:
            r[key + "_us_per_further_substep"] = round(slope, 3)
    res = dict(name=cfg["name"], workload=cfg["desc"], single_step_kernel="k_step (fused)" if fused else "k_cars + k_lidar",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, rows=rows)
    if not cfg.get("traffic"):
        # branching: mev_restore_map against a masked mev_restore, the same (env, field) grid
        snap = torch.empty(h.snapshot_size(), dtype=torch.uint8, device=dev)
        h.snapshot(snap, device=True)
        emap = torch.zeros(E, dtype=torch.int32, device=dev)
        mask = torch.ones(E, dtype=torch.uint8, device=dev)

        def maps():
            for c in range(CALLS):
                h.restore(snap, env_map=emap, device=True)

        def masks():
            for c in range(CALLS):
                h.restore(snap, env_mask=mask, device=True)

        maps()
        masks()
        torch.cuda.synchronize(dev)
        t_map, t_mask = [], []
        for _ in range(RUNS):
            t_mask.append(timed(masks) / CALLS)
            t_map.append(timed(maps) / CALLS)
        res["restore"] = dict(note="device pointers; each call also reads the snapshot header back to the host",
                              restore_map=stat(t_map), restore_mask=stat(t_mask))
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    res = dict(method="stream events around 50 calls (mev_step_sequence with and without the *_seq arrays, "
                      "mev_step_repeat(n = T), T mev_step calls with the plan's per-step actions), 5 runs each "
                      "(median, min-max), one process, one device; device pointers, auto-reset",
               library_variant=os.environ.get("MEV_LIB_VARIANT", ""), device=torch.cuda.get_device_name(0), shapes=[])
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], json.dumps(row), flush=True)
        if "restore" in r:
            print(r["name"], "restore", json.dumps(r["restore"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
