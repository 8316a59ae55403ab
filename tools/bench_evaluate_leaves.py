"""What the leaf observations of candidate plans (mev_evaluate_leaves) cost against the only route
to them without the call, by tools/bench_evaluate.py's method unchanged: the same two shapes (4096
envs x 8 agents x 64 beams with the team reward; 4096 x 1 x 64 with traffic at density 0.5), device
pointers, every output written, one session on one device, bench.py's clock settle and warm-up, the
time of 50 calls by stream events, five blocks each, alternating.  C = 4096 candidates, 64 per root.
For a plan length T in 2, 4, 8, 16:
  leaf      (a) mev_evaluate_leaves with every output and leaf_obs [C][N][obs_dim]
  pair      (b) mev_restore_map(roots) from the snapshot + mev_step_sequence with the three *_seq arrays
            and substeps -- its obs are the leaf observations; the closing mev_restore separately
  eval      (c) mev_evaluate_plans on the same inputs: (a) - (c) is what the leaves themselves cost
Also (a) with C = 16384 candidates from the same 4096-env handle.  The bar: (a)'s median below (b)'s
by more than the larger of the two block spreads (leaf_beats_pair_by_more_than_spread, per row).
    python tools/bench_evaluate_leaves.py [--out profiles/evaluate_leaves_sweep.json] [--only cfg3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_evaluate import CALLS, C_MANY, GAMMA, LENGTHS, PLANS, RUNS, SETTLE_MS, SHAPES, WARMUP, med, stat  # noqa: E402


def measure(cfg):
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R = cfg["E"], cfg["N"], cfg["R"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, use_team_reward=cfg.get("team", 0),
                   traffic_flow=cfg.get("traffic", 0), traffic_density=0.5, max_steps=2000, seed=0, device=0)
    D = h.D
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

    def eval_out(T, C, leaf):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        o = dict(returns=z((C, N), torch.float32), reward_seq=z((T, C, N), torch.float32),
                 done_seq=z((T, C, N), torch.uint8), status_seq=z((T, C, N), torch.uint8),
                 substeps=z(C, torch.int32), terminated=z(C, torch.uint8), truncated=z(C, torch.uint8))
        if leaf:
            o["leaf_obs"] = z((C, N, D), torch.float32)
        return o

    rows = []
    for T in LENGTHS:
        lout, eout, mout = eval_out(T, E, True), eval_out(T, E, False), eval_out(T, C_MANY, True)
        sout = dict(out, substeps=torch.zeros(E, dtype=torch.int32, device=dev),
                    **{k: torch.zeros_like(eout[k]) for k in ("reward_seq", "done_seq", "status_seq")})

        def put_back():
            h.restore(snap, device=True)

        def leaf_calls():
            for c in range(CALLS):
                h.evaluate_plans(acts[c % PLANS].data_ptr(), roots, 1.0 / 60.0, GAMMA, out=lout, device=True,
                                 candidates=E, length=T, leaf_obs=True)

        def eval_calls():
            for c in range(CALLS):
                h.evaluate_plans(acts[c % PLANS].data_ptr(), roots, 1.0 / 60.0, GAMMA, out=eout, device=True,
                                 candidates=E, length=T)

        def many_calls():
            for c in range(CALLS):
                h.evaluate_plans(acts_many[c % PLANS].data_ptr(), roots_many, 1.0 / 60.0, GAMMA, out=mout, device=True,
                                 candidates=C_MANY, length=T, leaf_obs=True)

        def pair_calls():
            for c in range(CALLS):
                h.restore(snap, env_map=roots, device=True)
                h.step_sequence(acts[c % PLANS].data_ptr(), 1.0 / 60.0, out=sout, device=True, length=T)

        def restore_calls():
            for c in range(CALLS):
                put_back()

        # warm every call of the timed blocks, and check that (a) and (b) give the same observations
        pair_calls()
        put_back()
        leaf_calls()
        eval_calls()
        many_calls()
        torch.cuda.synchronize(dev)
        same = None  # (traffic: the pair's calls advance the Philox counter, the spawns differ)
        if not cfg.get("traffic"):
            same = bool(torch.equal(lout["leaf_obs"].view(torch.int32), sout["obs"].view(torch.int32).reshape(E, N, D)))
        t_leaf, t_pair, t_rest, t_eval, t_many = [], [], [], [], []
        for _ in range(RUNS):
            put_back()
            t_leaf.append(timed(leaf_calls) / CALLS)
            t_pair.append(timed(pair_calls) / CALLS)
            t_rest.append(timed(restore_calls) / CALLS)
            t_eval.append(timed(eval_calls) / CALLS)
            t_many.append(timed(many_calls) / CALLS)
        torch.cuda.synchronize(dev)
        a, b = stat(t_leaf), stat(t_pair)
        rows.append(dict(
            length=T, candidates=E, leaf=a, pair=b, closing_restore=stat(t_rest), eval=stat(t_eval),
            ratio_pair_over_leaf=round(b["ms"] / a["ms"], 4),
            leaf_beats_pair_by_more_than_spread=bool(b["ms"] - a["ms"] > max(a["spread"], b["spread"])),
            leaf_minus_eval_us=round((a["ms"] - med(t_eval)) * 1e3, 3),
            leaf_us_per_candidate=round(a["ms"] * 1e3 / E, 5),
            leaf_obs_equal_pair_obs=same,
            many=dict(candidates=C_MANY, **stat(t_many), us_per_candidate=round(med(t_many) * 1e3 / C_MANY, 5)),
            mean_substeps=round(float(lout["substeps"].float().mean()), 3)))
    lo, hi = rows[0], rows[-1]
    for key in ("leaf", "pair", "eval"):
        slope = (hi[key]["ms"] - lo[key]["ms"]) / (hi["length"] - lo["length"]) * 1e3
        for r in rows:
            r[key + "_us_per_further_substep"] = round(slope, 3)
    res = dict(name=cfg["name"], workload=cfg["desc"], obs_dim=D, roots="arange(E) // 64 * 64 (64 candidates per root)",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, gamma=GAMMA,
               rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_leaves_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate_leaves.py needs a HIP device")
    res = dict(method="stream events around 50 calls (mev_evaluate_leaves with every output; mev_restore_map + "
                      "mev_step_sequence with the *_seq arrays; the closing mev_restore; mev_evaluate_plans; "
                      "mev_evaluate_leaves with 16384 candidates), 5 alternated blocks each (median, min-max), one "
                      "process, one device; device pointers",
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
