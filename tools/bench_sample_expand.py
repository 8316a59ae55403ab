"""What sampled continuations below the root cost with the draw, the pooled roots and the kept stop
states in one call (mev_sample_expand_plans) against the only way there without it: the draw in
eager torch followed by mev_expand_plans.

The method of tools/bench_evaluate.py, unchanged: BASELINE config 3 (4096 envs x 8 agents x 64
beams, team reward) and config 4 (4096 x 1 x 64, traffic at density 0.5); device pointers, one
session, one device; the live batch is a handle after bench.py's clock settle and warm-up; every
output written; the time of 50 calls by stream events, five blocks each, alternating.  G groups of
K candidates, plan length T, without and with leaf_obs.  A first level (mev_sample_expand_plans
from the live batch, group g from env g * (E // G), candidate c into slot c of a pool) fills the
slots the timed legs start from: group g of the second level starts from slot g * K.
  a  mev_sample_expand_plans from those slots, candidate c into slot C + c: a tree's second level
  b  the same level as it is written without the call, on the same handle, stream and pool
     contents: randn, index_select of the groups' mean and sigma, scale, add, clamp, then
     mev_expand_plans on those actions
  c  mev_sample_plans from the live batch on the same distribution (a - c: what pooled roots and
     keeping cost over the sampled call)
The run asserts that a's outputs equal mev_expand_plans(actions_out) bit for bit.
    python tools/bench_sample_expand.py [--out profiles/sample_expand_sweep.json] [--only cfg3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_evaluate import CALLS, GAMMA, PLANS, RUNS, SETTLE_MS, SHAPES, WARMUP, med, stat  # noqa: E402

# (groups, samples, length) per shape; each without and with leaf_obs
CASES = {"cfg3": [(64, 64, 4), (64, 64, 8), (4096, 4, 4), (4096, 4, 8)], "cfg4": [(64, 64, 4)]}
LEAF = {"cfg3": (False, True), "cfg4": (False, True)}


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
        pool = h.pool(2 * C)
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        live_roots = (torch.arange(G, dtype=torch.int32, device=dev) * (E // G)).contiguous()
        roots = (torch.arange(G, dtype=torch.int32, device=dev) * K).contiguous()  # slot of group g's first child
        roots_c = roots.repeat_interleave(K).contiguous()
        group = torch.arange(C, device=dev) // K
        slots0 = torch.arange(C, dtype=torch.int32, device=dev).contiguous()
        slots1 = (slots0 + C).contiguous()
        mean = (torch.rand((T, G, N, 2), device=dev, generator=g) - 0.3).contiguous()
        sigma = torch.full((T, G, N, 2), 0.5, device=dev)
        kw = dict(dt=1.0 / 60.0, gamma=GAMMA, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=1234, device=True, groups=G, length=T)
        # the first level: every slot in [0, C) holds a stop state
        h.sample_plans(mean, sigma, live_roots, K, counter=1 << 20, out={}, dst=pool, dst_slots=slots0, **kw)
        torch.cuda.synchronize(dev)
        assert bool(pool.get_state(slots0.cpu().numpy())[2].all())
        for leaf in LEAF[cfg["name"]]:

            def eval_out(actions):
                o = dict(returns=z((C, N)), reward_seq=z((T, C, N)), done_seq=z((T, C, N), torch.uint8),
                         status_seq=z((T, C, N), torch.uint8), substeps=z(C, torch.int32), terminated=z(C, torch.uint8),
                         truncated=z(C, torch.uint8))
                if leaf:
                    o["leaf_obs"] = z((C, N, h.D))
                if actions:
                    o["actions_out"] = z((T, C, N, 2))
                return o

            oa, ob, oc, ox = eval_out(True), eval_out(False), eval_out(True), eval_out(False)

            def a_calls():
                for c in range(CALLS):
                    h.sample_plans(mean, sigma, roots, K, counter=c, leaf_obs=leaf, out=oa, src=pool, dst=pool,
                                   dst_slots=slots1, counter_offset=T, **kw)

            def b_calls():
                for c in range(CALLS):
                    eps = torch.randn((T, C, N, 2), device=dev, generator=g)
                    a = torch.clamp(mean.index_select(1, group) + sigma.index_select(1, group) * eps, -1.0, 1.0)
                    h.expand_plans(a, roots_c, pool, slots1, pool, T, leaf, 1.0 / 60.0, GAMMA, out=ob, device=True,
                                   candidates=C, length=T)

            def c_calls():
                for c in range(CALLS):
                    h.sample_plans(mean, sigma, live_roots, K, counter=c, leaf_obs=leaf, out=oc, **kw)

            for fn in (a_calls, b_calls, c_calls):  # warm every call of the timed blocks
                fn()
            # a computes and stores what mev_expand_plans does on the actions it reports (oa holds counter
            # CALLS - 1's candidates): the same call on those actions into the same slots, outputs and slots compared
            a_calls()
            torch.cuda.synchronize(dev)
            kept = pool.get_state(slots1.cpu().numpy())
            h.expand_plans(oa["actions_out"], roots_c, pool, slots1, pool, T, leaf, 1.0 / 60.0, GAMMA, out=ox, device=True,
                           candidates=C, length=T)
            torch.cuda.synchronize(dev)
            for k in ox:
                assert torch.equal(oa[k].view(torch.uint8), ox[k].view(torch.uint8)), k
            again = pool.get_state(slots1.cpu().numpy())
            assert bool(kept[2].all()) and bool(again[2].all())
            for name in kept[0]:
                x, y = kept[0][name], again[0][name]
                if name.startswith("npc_") and name != "npc_count":  # (beyond a slot's count: unspecified)
                    live = np.arange(x.shape[1])[None, :] < kept[0]["npc_count"][:, None]
                    x, y = x[live], y[live]
                assert x.tobytes() == y.tobytes(), name
            ta, tb, tc = [], [], []
            for _ in range(RUNS):
                ta.append(timed(a_calls) / CALLS)
                tb.append(timed(b_calls) / CALLS)
                tc.append(timed(c_calls) / CALLS)
            torch.cuda.synchronize(dev)
            sa, sb, sc = stat(ta), stat(tb), stat(tc)
            margin = max(sa["spread"], sb["spread"])
            rows.append(dict(
                groups=G, samples=K, candidates=C, length=T, leaf_obs=leaf, a_sample_expand_from_pool=sa,
                b_eager_draw_then_expand=sb, c_sample_plans_from_live=sc, b_minus_a_us=round((med(tb) - med(ta)) * 1e3, 3),
                larger_spread_a_b_us=round(margin * 1e3, 3), a_below_b_by_more_than_spread=bool(med(tb) - med(ta) > margin),
                a_minus_c_us=round((med(ta) - med(tc)) * 1e3, 3),
                larger_spread_a_c_us=round(max(sa["spread"], sc["spread"]) * 1e3, 3),
                a_outputs_and_slots_equal_expand_plans=True, mean_substeps_a=round(float(oa["substeps"].float().mean()), 3)))
        pool.close()
    res = dict(name=cfg["name"], workload=cfg["desc"],
               roots="first level: group g from env g * (E // G) into slots [0, C); timed second level: group g from slot "
                     "g * K into slots [C, 2C)",
               calls_per_measurement=CALLS, runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, gamma=GAMMA, rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_expand_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_expand.py needs a HIP device")
    res = dict(method="stream events around 50 calls (a: mev_sample_expand_plans pool -> pool, one slot per candidate; b: "
                      "eager torch draw, then mev_expand_plans pool -> pool; c: mev_sample_plans from the live batch), every "
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
