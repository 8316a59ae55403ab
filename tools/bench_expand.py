"""What keeping candidates' stop states in a device pool (mev_expand_plans) costs, and what the
second level of a tree costs with it against the only way to reach it without.

The method of tools/bench_evaluate.py, unchanged: BASELINE config 3 (4096 envs x 8 agents x 64
beams, team reward) and config 4 (4096 x 1 x 64, traffic at density 0.5); device pointers, one
session, one device; the live batch is a handle after bench.py's clock settle and warm-up; C = 4096
candidates, 64 per root (roots = arange(E) // 64 * 64), every output written; the time of 50 calls by
stream events, five blocks each, alternating.  For a plan length T in 2, 4, 8, without and with
leaf_obs:
  a  mev_expand_plans from the live batch into slots [0, C) of a pool
  b  mev_expand_plans from those slots, one per candidate, into slots [C, 2C): a tree's second level
  c  mev_evaluate_plans / mev_evaluate_leaves at T on a's inputs (a - c: what the stores cost)
  d  mev_evaluate_plans / mev_evaluate_leaves at 2T from the live batch: the only way to the second
     level that leaves the batch alone without a pool (the prefix replayed)
    python tools/bench_expand.py [--out profiles/expand_sweep.json] [--only cfg3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_evaluate import CALLS, GAMMA, PLANS, RUNS, SETTLE_MS, SHAPES, WARMUP, med, stat  # noqa: E402

LENGTHS = (2, 4, 8)


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
    tmax = 2 * max(LENGTHS)
    acts = torch.rand((PLANS, tmax, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
    h.reset(device=True)
    n_settle = 0
    t_end = time.perf_counter() + SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            h.step(acts[n_settle % PLANS, 0].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(WARMUP):
        h.step(acts[t % PLANS, t % tmax].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)
    C = E
    roots = (torch.arange(E, dtype=torch.int32, device=dev) // 64 * 64).contiguous()
    slots0 = torch.arange(C, dtype=torch.int32, device=dev).contiguous()
    slots1 = (slots0 + C).contiguous()
    pool = h.pool(2 * C)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def eval_out(T, leaf):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        o = dict(returns=z((C, N), torch.float32), reward_seq=z((T, C, N), torch.float32),
                 done_seq=z((T, C, N), torch.uint8), status_seq=z((T, C, N), torch.uint8),
                 substeps=z(C, torch.int32), terminated=z(C, torch.uint8), truncated=z(C, torch.uint8))
        if leaf:
            o["leaf_obs"] = z((C, N, h.D), torch.float32)
        return o

    rows = []
    for T in LENGTHS:
        for leaf in (False, True):
            oa, ob, oc, od = eval_out(T, leaf), eval_out(T, leaf), eval_out(T, leaf), eval_out(2 * T, leaf)

            def a_calls():
                for c in range(CALLS):
                    h.expand_plans(acts[c % PLANS].data_ptr(), roots, pool, slots0, None, 0, leaf, 1.0 / 60.0, GAMMA,
                                   out=oa, device=True, candidates=C, length=T)

            def b_calls():
                for c in range(CALLS):
                    h.expand_plans(acts[c % PLANS, T:].data_ptr(), slots0, pool, slots1, pool, T, leaf, 1.0 / 60.0, GAMMA,
                                   out=ob, device=True, candidates=C, length=T)

            def c_calls():
                for c in range(CALLS):
                    h.evaluate_plans(acts[c % PLANS].data_ptr(), roots, 1.0 / 60.0, GAMMA, out=oc, device=True,
                                     candidates=C, length=T, leaf_obs=leaf)

            def d_calls():
                for c in range(CALLS):
                    h.evaluate_plans(acts[c % PLANS].data_ptr(), roots, 1.0 / 60.0, GAMMA, out=od, device=True,
                                     candidates=C, length=2 * T, leaf_obs=leaf)

            # warm every call of the timed blocks (a fills the slots b starts from), and check that
            # the kept states change nothing of what the evaluation computes
            a_calls()
            b_calls()
            c_calls()
            d_calls()
            torch.cuda.synchronize(dev)
            same = all(bool(torch.equal(oa[k].view(torch.uint8), oc[k].view(torch.uint8))) for k in oa)
            ta, tb, tc, td = [], [], [], []
            for _ in range(RUNS):
                ta.append(timed(a_calls) / CALLS)
                tb.append(timed(b_calls) / CALLS)
                tc.append(timed(c_calls) / CALLS)
                td.append(timed(d_calls) / CALLS)
            torch.cuda.synchronize(dev)
            sb, sd = stat(tb), stat(td)
            margin = max(sb["spread"], sd["spread"])
            rows.append(dict(
                length=T, leaf_obs=leaf, candidates=C, a_expand_from_live=stat(ta), b_expand_from_pool=sb,
                c_evaluate_T=stat(tc), d_evaluate_2T=sd, store_cost_us=round((med(ta) - med(tc)) * 1e3, 3),
                b_minus_c_us=round((med(tb) - med(tc)) * 1e3, 3), d_minus_b_us=round((med(td) - med(tb)) * 1e3, 3),
                larger_spread_us=round(margin * 1e3, 3), b_below_d_by_more_than_spread=bool(med(td) - med(tb) > margin),
                a_outputs_equal_c_outputs=same, mean_substeps_a=round(float(oa["substeps"].float().mean()), 3),
                mean_substeps_b=round(float(ob["substeps"].float().mean()), 3)))
    res = dict(name=cfg["name"], workload=cfg["desc"], roots="arange(E) // 64 * 64 (64 candidates per root)",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, gamma=GAMMA,
               rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    pool.close()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_expand.py needs a HIP device")
    res = dict(method="stream events around 50 calls (a: mev_expand_plans live -> pool; b: pool -> pool, one slot per "
                      "candidate; c: mev_evaluate_plans / _leaves at T; d: the same at 2T), every output, 5 alternated "
                      "blocks each (median, min-max), one process, one device; device pointers",
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
