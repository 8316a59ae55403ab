"""What scoring candidate plans (mev_evaluate_plans) costs against what a planner pays without it.

Shapes: BASELINE config 3 (4096 envs x 8 agents x 64 beams, team reward) and config 4
(4096 x 1 x 64, traffic at density 0.5); device pointers, one session, one device.  The live
batch is a handle after a clock settle and a warm-up as bench.py does; its snapshot is taken
once.  C = 4096 candidates, 64 per root (roots = arange(E) // 64 * 64).  For a plan length T in
2, 4, 8, 16, the time of 50 calls by stream events, five blocks each, alternating:
  eval      mev_evaluate_plans with every output (returns, the three *_seq arrays, substeps, flags)
  pair      what the same result costs without it: mev_restore_map(roots) from the snapshot, then
            mev_step_sequence with the three *_seq arrays and substeps (no auto-reset)
  restore   the closing mev_restore that puts the batch back after a pair (reported separately:
            a planner pays it once per iteration, after its last rollout)
Before each eval block the batch is put back (untimed), so both start from the same state.
Also C = 16384 candidates from the same 4096-env handle (the pair cannot do this at all),
reported per candidate.
    python tools/bench_evaluate.py [--out profiles/evaluate_sweep.json] [--only cfg3]"""
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
PLANS = 4  # distinct plan sets cycled through the 50 calls
C_MANY = 16384
GAMMA = 0.97


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
    acts_many = torch.rand((PLANS, tmax, C_MANY, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
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
    # the live batch, and its snapshot (what the pair branches from and is put back to)
    snap = torch.empty(h.snapshot_size(), dtype=torch.uint8, device=dev)
    h.snapshot(snap, device=True)
    roots = (torch.arange(E, dtype=torch.int32, device=dev) // 64 * 64).contiguous()
    roots_many = (torch.arange(C_MANY, dtype=torch.int32, device=dev) % E // 64 * 64).contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def eval_out(T, C):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        return dict(returns=z((C, N), torch.float32), reward_seq=z((T, C, N), torch.float32),
                    done_seq=z((T, C, N), torch.uint8), status_seq=z((T, C, N), torch.uint8),
                    substeps=z(C, torch.int32), terminated=z(C, torch.uint8), truncated=z(C, torch.uint8))

    rows = []
    for T in LENGTHS:
        eout, mout = eval_out(T, E), eval_out(T, C_MANY)
        sout = dict(out, substeps=torch.zeros(E, dtype=torch.int32, device=dev),
                    **{k: torch.zeros_like(eout[k]) for k in ("reward_seq", "done_seq", "status_seq")})

        def put_back():
            h.restore(snap, device=True)

        def eval_calls():
            for c in range(CALLS):
                h.evaluate_plans(acts[c % PLANS].data_ptr(), roots, 1.0 / 60.0, GAMMA, out=eout, device=True,
                                 candidates=E, length=T)

        def many_calls():
            for c in range(CALLS):
                h.evaluate_plans(acts_many[c % PLANS].data_ptr(), roots_many, 1.0 / 60.0, GAMMA, out=mout, device=True,
                                 candidates=C_MANY, length=T)

        def pair_calls():
            for c in range(CALLS):
                h.restore(snap, env_map=roots, device=True)
                h.step_sequence(acts[c % PLANS].data_ptr(), 1.0 / 60.0, out=sout, device=True, length=T)

        def restore_calls():
            for c in range(CALLS):
                put_back()

        # warm every call of the timed blocks, and check that the two compute the same rows
        pair_calls()
        put_back()
        eval_calls()
        many_calls()
        torch.cuda.synchronize(dev)
        same = None  # (traffic: the pair's calls advance the Philox counter, the spawns differ)
        if not cfg.get("traffic"):
            same = all(bool(torch.equal(eout[k], sout[k])) for k in ("done_seq", "status_seq", "substeps")) and \
                bool(torch.equal(eout["reward_seq"].view(torch.int32), sout["reward_seq"].view(torch.int32)))
        t_eval, t_pair, t_rest, t_many = [], [], [], []
        for _ in range(RUNS):
            put_back()
            t_eval.append(timed(eval_calls) / CALLS)
            t_pair.append(timed(pair_calls) / CALLS)
            t_rest.append(timed(restore_calls) / CALLS)
            t_many.append(timed(many_calls) / CALLS)
        torch.cuda.synchronize(dev)
        rows.append(dict(
            length=T, candidates=E, eval=stat(t_eval), pair=stat(t_pair), closing_restore=stat(t_rest),
            ratio_pair_over_eval=round(med(t_pair) / med(t_eval), 4),
            eval_not_slower_than_pair=bool(med(t_eval) <= med(t_pair)),
            eval_us_per_candidate=round(med(t_eval) * 1e3 / E, 5),
            eval_rows_equal_pair_rows=same,
            many=dict(candidates=C_MANY, **stat(t_many), us_per_candidate=round(med(t_many) * 1e3 / C_MANY, 5)),
            mean_substeps=round(float(eout["substeps"].float().mean()), 3)))
    lo, hi = rows[0], rows[-1]
    for key in ("eval", "pair"):
        slope = (hi[key]["ms"] - lo[key]["ms"]) / (hi["length"] - lo["length"]) * 1e3
        for r in rows:
            r[key + "_us_per_further_substep"] = round(slope, 3)
    res = dict(name=cfg["name"], workload=cfg["desc"], roots="arange(E) // 64 * 64 (64 candidates per root)",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, gamma=GAMMA, rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py needs a HIP device")
    res = dict(method="stream events around 50 calls (mev_evaluate_plans with every output; mev_restore_map + "
                      "mev_step_sequence with the *_seq arrays; the closing mev_restore; mev_evaluate_plans with 16384 "
                      "candidates), 5 alternated blocks each (median, min-max), one process, one device; device pointers",
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
