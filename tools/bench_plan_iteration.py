"""What one iteration of a sampling planner (CEM / MPPI) costs with the sampling and the refit inside
the library (mev_sample_plans + mev_update_plans) against the same iteration written in eager torch
around mev_evaluate_plans.

The method of tools/bench_evaluate.py, unchanged: BASELINE config 3 (4096 envs x 8 agents x 64
beams, team reward) and config 4 (4096 x 1 x 64, traffic at density 0.5); device pointers, one
session, one device; the live batch is a handle after bench.py's clock settle and warm-up; every
output written; the time of 50 calls by stream events, five blocks each, alternating.  G groups of
K candidates (group g starts from env g * (E // G)), plan length T:
  a   mev_sample_plans + mev_update_plans (softmax over the candidates' summed returns)
  b   the same iteration in eager torch on the same handle and stream: randn, gather of the groups'
      mean and sigma, scale, add, clamp, mev_evaluate_plans, sum, softmax, weighted mean and std
  c1  mev_sample_plans alone
  c2  mev_evaluate_plans on pre-made actions (c1's actions_out)
The run asserts that a's evaluation outputs equal mev_evaluate_plans(actions_out) bit for bit.
    python tools/bench_plan_iteration.py [--out profiles/plan_iteration_sweep.json] [--only cfg3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_evaluate import CALLS, GAMMA, PLANS, RUNS, SETTLE_MS, SHAPES, WARMUP, med, stat  # noqa: E402

# (groups, samples, length) per shape
CASES = {"cfg3": [(64, 64, 4), (64, 64, 8), (4096, 4, 4), (4096, 4, 8)], "cfg4": [(64, 64, 4)]}
TEMPERATURE = 2.0
EVAL_KEYS = ("returns", "reward_seq", "done_seq", "status_seq", "substeps", "terminated", "truncated")


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
    acts = torch.rand((PLANS, 16, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
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
        h.step(acts[t % PLANS, t % 16].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    rows = []
    for G, K, T in CASES[cfg["name"]]:
        C = G * K
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)

        def eval_out():
            return dict(returns=z((C, N)), reward_seq=z((T, C, N)), done_seq=z((T, C, N), torch.uint8),
                        status_seq=z((T, C, N), torch.uint8), substeps=z(C, torch.int32), terminated=z(C, torch.uint8),
                        truncated=z(C, torch.uint8))

        roots = (torch.arange(G, dtype=torch.int32, device=dev) * (E // G)).contiguous()
        roots_c = roots.repeat_interleave(K).contiguous()
        group = torch.arange(C, device=dev) // K
        mean = (torch.rand((T, G, N, 2), device=dev, generator=g) - 0.3).contiguous()
        sigma = torch.full((T, G, N, 2), 0.5, device=dev)
        oa, ob, oc1, oc2 = (eval_out() for _ in range(4))
        oa["actions_out"], oc1["actions_out"] = z((T, C, N, 2)), z((T, C, N, 2))
        ua = dict(new_mean=z((T, G, N, 2)), new_sigma=z((T, G, N, 2)), best=z(G, torch.int32), best_score=z(G),
                  weights=z(C))
        kw = dict(dt=1.0 / 60.0, gamma=GAMMA, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=1234, device=True, groups=G, length=T)
        tb_out = {}

        def a_calls():
            for c in range(CALLS):
                h.sample_plans(mean, sigma, roots, K, counter=c, out=oa, **kw)
                h.update_plans(oa["actions_out"], K, returns=oa["returns"], mode="softmax", temperature=TEMPERATURE,
                               out=ua, device=True, groups=G, length=T)

        def b_calls():
            for c in range(CALLS):
                eps = torch.randn((T, C, N, 2), device=dev, generator=g)
                a = torch.clamp(mean.index_select(1, group) + sigma.index_select(1, group) * eps, -1.0, 1.0)
                h.evaluate_plans(a, roots_c, 1.0 / 60.0, GAMMA, out=ob, device=True, candidates=C, length=T)
                w = torch.softmax(ob["returns"].sum(1).view(G, K) / TEMPERATURE, dim=1)[None, :, :, None, None]
                a5 = a.view(T, G, K, N, 2)
                m = (w * a5).sum(2)
                d = a5 - m[:, :, None]
                tb_out["new_mean"], tb_out["new_sigma"] = m, (w * d * d).sum(2).sqrt()

        def c1_calls():
            for c in range(CALLS):
                h.sample_plans(mean, sigma, roots, K, counter=c, out=oc1, **kw)

        def c2_calls():
            for c in range(CALLS):
                h.evaluate_plans(oc1["actions_out"], roots_c, 1.0 / 60.0, GAMMA, out=oc2, device=True, candidates=C,
                                 length=T)

        for fn in (a_calls, b_calls, c1_calls, c2_calls):  # warm every call of the timed blocks
            fn()
        torch.cuda.synchronize(dev)
        # the sampled call computes what mev_evaluate_plans computes on the actions it reports
        # (oc1 and oa hold counter CALLS - 1's candidates, oc2 was run on oc1's actions_out)
        for k in EVAL_KEYS:
            assert torch.equal(oc1[k].view(torch.uint8), oc2[k].view(torch.uint8)), k
            assert torch.equal(oa[k].view(torch.uint8), oc2[k].view(torch.uint8)), k
        assert torch.equal(oa["actions_out"], oc1["actions_out"])
        ta, tb, tc1, tc2 = [], [], [], []
        for _ in range(RUNS):
            ta.append(timed(a_calls) / CALLS)
            tb.append(timed(b_calls) / CALLS)
            tc1.append(timed(c1_calls) / CALLS)
            tc2.append(timed(c2_calls) / CALLS)
        torch.cuda.synchronize(dev)
        sa, sb, s1, s2 = stat(ta), stat(tb), stat(tc1), stat(tc2)
        margin = max(sa["spread"], sb["spread"])
        rows.append(dict(
            groups=G, samples=K, candidates=C, length=T, a_sample_update=sa, b_eager_torch=sb, c1_sample_plans=s1,
            c2_evaluate_plans=s2, b_minus_a_us=round((med(tb) - med(ta)) * 1e3, 3),
            larger_spread_a_b_us=round(margin * 1e3, 3), a_below_b_by_more_than_spread=bool(med(tb) - med(ta) > margin),
            c1_minus_c2_us=round((med(tc1) - med(tc2)) * 1e3, 3),
            larger_spread_c_us=round(max(s1["spread"], s2["spread"]) * 1e3, 3),
            c_level_within_spreads=bool(abs(med(tc1) - med(tc2)) <= max(s1["spread"], s2["spread"])),
            a_outputs_equal_evaluate_plans=True, mean_substeps=round(float(oa["substeps"].float().mean()), 3)))
    res = dict(name=cfg["name"], workload=cfg["desc"], roots="group g starts from env g * (E // G)",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, gamma=GAMMA,
               temperature=TEMPERATURE, rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_iteration_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_iteration.py needs a HIP device")
    res = dict(method="stream events around 50 iterations (a: mev_sample_plans + mev_update_plans softmax; b: eager torch "
                      "around mev_evaluate_plans; c1: mev_sample_plans; c2: mev_evaluate_plans on pre-made actions), every "
                      "output, 5 alternated blocks each (median, min-max), one process, one device; device pointers",
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
