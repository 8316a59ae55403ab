"""What a policy per agent slot inside a closed-loop rollout (mev_rollout_policies) costs against what a user runs
without it.

tools/bench_rollout_repeat.py's method, unchanged: device pointers, auto-reset, every *_seq output plus value_seq and
substeps_seq, a clock settle and a warm-up as bench.py does, then for each assignment and repeat the time of CALLS
rollouts of T decisions x n sub-steps by stream events, five blocks each, alternating:
  multi     (a) mev_rollout_policies with P policies and the assignment
  eager     (b) the same semantics without it: per decision an eager torch forward pass (no_grad) of EACH of the P
            policies -- trunk, actor and value head -- over all rows, a torch.gather by `assign`, a clamp into the
            preallocated action row, and mev_step_repeat (auto-reset) into the rows of the same tensors
  single    (c) mev_rollout_policy_repeat with one policy on the same build: other semantics, for orientation only
Assignments: P = 1; P = 2 with the agents of every env split 4 / 4; P = 2 by env parity (every env has one policy);
P = 8, one policy per agent.  A shape counts as a gain only where (a) is below (b) by more than both blocks' spreads;
a loss is reported as one.  Also recorded: the register figures of every k_rollout instantiation from the library's
code object and, with --parent-lib, from the library of the commit before; and, with --merge NAME=FILE, other runs'
JSON (the unchanged call timed on both builds in the same session) under "unchanged_calls".
    python tools/bench_rollout_multi.py [--out profiles/rollout_multi_sweep.json] [--only NAME] [--parent-lib SO]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_rollout_repeat as BR  # noqa: E402  (the method: its constants, statistics and code-object reader)

BIG = dict(E=4096, N=8, R=64, D=95, team=1, hidden=(64, 64), T=16)
ASSIGN = ("one_policy", "split_4_4", "env_parity", "one_per_agent")
SHAPES = [
    dict(BIG, name="cfg3_64", desc="4096 envs x 8 agents x 64 beams, team reward, policies 95-64-64-2 with value heads",
         repeats=(1, 4), assigns=ASSIGN),
    dict(BIG, name="small", desc="64 envs x 8 agents x 64 beams, team reward, policies 95-64-64-2 with value heads", E=64,
         repeats=(4,), assigns=("split_4_4",)),
]


def assignment(kind, E, N):
    """(P, assign [E][N] uint8 as nested lists' numpy array)"""
    import numpy as np
    e, i = np.meshgrid(np.arange(E), np.arange(N), indexing="ij")
    if kind == "one_policy":
        return 1, np.zeros((E, N), np.uint8)
    if kind == "split_4_4":
        return 2, (i >= N // 2).astype(np.uint8)
    if kind == "env_parity":
        return 2, (e % 2).astype(np.uint8)
    if kind == "one_per_agent":
        return N, i.astype(np.uint8)
    raise KeyError(kind)


def measure(cfg):
    import numpy as np
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R, D, T = cfg["E"], cfg["N"], cfg["R"], cfg["D"], cfg["T"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, obs_dim=D, use_team_reward=cfg.get("team", 0),
                   traffic_flow=0, traffic_density=0.5, max_steps=2000, seed=0, device=0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    h.set_stream(st.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    acts = torch.rand((4, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
    h.reset(device=True)
    n_settle = 0
    t_end = time.perf_counter() + BR.SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            h.step(acts[n_settle % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(BR.WARMUP):
        h.step(acts[t % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)

    # 8 policies: weights ~ N(0, 1 / in), a positive throttle bias (the cars move), a value head on each trunk
    torch.manual_seed(7)
    nn = torch.nn
    dims = (D,) + tuple(cfg["hidden"]) + (2,)
    nets = []
    for _ in range(mev._capi.MEV_MAX_ROLLOUT_POLICIES):
        layers = []
        for i, o in zip(dims[:-1], dims[1:]):
            lin = nn.Linear(i, o)
            with torch.no_grad():
                lin.weight.normal_(0.0, i ** -0.5)
                lin.bias.normal_(0.0, 0.1)
            layers += [lin, nn.ReLU()]
        trunk = nn.Sequential(*layers[:-2]).to(dev)  # ... up to the last hidden layer's ReLU
        actor = layers[-2].to(dev)
        critic = nn.Linear(dims[-2], 1).to(dev)
        with torch.no_grad():
            actor.bias.copy_(torch.tensor([0.6, 0.0]))
        lins = [m for m in trunk if isinstance(m, nn.Linear)] + [actor]
        pol = h.policy([m.weight.detach() for m in lins], [m.bias.detach() for m in lins], device=True)
        pol.set_value_head(critic.weight.detach().reshape(-1), critic.bias.detach(), device=True)
        nets.append(dict(trunk=trunk, actor=actor, critic=critic, pol=pol))
    lo_t, hi_t = torch.tensor([-1.0, -1.0], device=dev), torch.tensor([1.0, 1.0], device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    seq = dict(obs_seq=z((T, E, N, D), torch.float32), actions_seq=z((T, E, N, 2), torch.float32),
               mean_seq=z((T, E, N, 2), torch.float32), reward_seq=z((T, E, N), torch.float32),
               done_seq=z((T, E, N), torch.uint8), status_seq=z((T, E, N), torch.uint8),
               terminated_seq=z((T, E), torch.uint8), truncated_seq=z((T, E), torch.uint8),
               value_seq=z((T + 1, E, N), torch.float32), substeps_seq=z((T, E), torch.int32))
    step_out = [dict(obs=seq["obs_seq"][t], reward=seq["reward_seq"][t], done=seq["done_seq"][t],
                     status=seq["status_seq"][t], terminated=seq["terminated_seq"][t],
                     truncated=seq["truncated_seq"][t], agents_alive=out["agents_alive"], step=out["step"],
                     substeps=seq["substeps_seq"][t]) for t in range(T)]
    act_ptr = [seq["actions_seq"][t].data_ptr() for t in range(T)]
    first_obs = torch.zeros((E, N, D), dtype=torch.float32, device=dev)

    rows = []
    for kind in cfg["assigns"]:
        P, assign_np = assignment(kind, E, N)
        assign = torch.as_tensor(assign_np).to(dev)
        used = nets[:P]
        pols = [u["pol"] for u in used]
        idx_v = assign.view(1, E * N).long()               # gather index over the stacked policies' rows
        idx_mu = idx_v.view(1, E * N, 1).expand(1, E * N, 2)
        distinct = float(np.mean([len(set(r.tolist())) for r in assign_np]))
        for n in cfg["repeats"]:
            calls = max(2, BR.SUBSTEPS_PER_BLOCK // (T * n))

            def multi_calls():
                for _ in range(calls):
                    h.rollout_policies(pols, assign, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True, repeat=n)

            def forward(obs, row):
                x = obs.view(E * N, D)
                hid = [u["trunk"](x) for u in used]
                vs = torch.stack([u["critic"](hd).view(E * N) for u, hd in zip(used, hid)])
                seq["value_seq"][row].copy_(vs.gather(0, idx_v).view(E, N))
                return hid

            def eager_calls():
                with torch.no_grad():
                    for _ in range(calls):
                        obs = first_obs
                        for t in range(T):
                            hid = forward(obs, t)
                            mus = torch.stack([u["actor"](hd) for u, hd in zip(used, hid)])
                            torch.clamp(mus.gather(0, idx_mu).view(E, N, 2), lo_t, hi_t, out=seq["actions_seq"][t])
                            h.step_repeat(act_ptr[t], n, 1.0 / 60.0, out=step_out[t], auto_reset=True, device=True)
                            obs = seq["obs_seq"][t]
                        forward(obs, T)
                        first_obs.copy_(obs)  # (the next rollout's first observation, as a user keeps it)

            def single_calls():
                for _ in range(calls):
                    h.rollout_policy(pols[0], T, 1.0 / 60.0, auto_reset=True, out=seq, device=True, repeat=n)

            h.get_outputs(dict(obs=first_obs), device=True)
            multi_calls(), eager_calls(), single_calls()  # warm every call of the timed blocks
            torch.cuda.synchronize(dev)
            ta, tb, tc = [], [], []
            for _ in range(BR.RUNS):
                ta.append(timed(multi_calls) / calls)
                h.get_outputs(dict(obs=first_obs), device=True)
                tb.append(timed(eager_calls) / calls)
                tc.append(timed(single_calls) / calls)
            a, b, c = BR.stat(ta, T, n), BR.stat(tb, T, n), BR.stat(tc, T, n)
            gain = b["min_max"][0] - a["min_max"][1] > 0 and b["ms"] - a["ms"] > max(a["spread"], b["spread"])
            loss = a["ms"] - b["ms"] > max(a["spread"], b["spread"])
            rows.append(dict(assignment=kind, policies=P, distinct_policies_per_env=distinct, decisions=T, repeat=n,
                             rollouts_per_block=calls, multi_call=a, eager=b, single_policy_call=c,
                             ratio_eager_over_multi=round(b["ms"] / a["ms"], 4),
                             us_per_decision_over_single=round(a["us_per_decision"] - c["us_per_decision"], 3),
                             verdict="gain" if gain else "loss" if loss else "tie"))
    res = dict(name=cfg["name"], workload=cfg["desc"], rollout_row=h.rollout_row(), runs=BR.RUNS,
               clock_settle_steps=n_settle, warmup_steps=BR.WARMUP, rows=rows)
    for u in nets:
        u["pol"].close()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_multi_sweep.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-lib", default="", help="the library built from the commit before: its register figures")
    ap.add_argument("--merge", action="append", default=[], metavar="NAME=FILE",
                    help="another run's JSON (or JSON-lines) output, stored under unchanged_calls[NAME]")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_multi.py needs a HIP device")
    import pkgload
    mev = pkgload.load()
    res = dict(method="stream events around blocks of 512 sub-steps (mev_rollout_policies with every *_seq output, "
                      "value_seq and substeps_seq; an eager torch forward of each listed policy's trunk, actor and value "
                      "head over all rows, a gather by assign, a clamp and mev_step_repeat per decision into the same "
                      "tensors; mev_rollout_policy_repeat with one policy), 5 alternated blocks each (median, min-max), "
                      "one process, one device; device pointers, auto-reset",
               device=torch.cuda.get_device_name(0), kernels=BR.kernel_resources(mev._capi.LIB_PATH), shapes=[])
    if a.parent_lib:
        res["kernels_parent"] = BR.kernel_resources(a.parent_lib)
        if res["kernels"] and res["kernels_parent"]:
            res["kernels_unchanged"] = all(res["kernels"].get(k) == v for k, v in res["kernels_parent"].items())
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], "row", r["rollout_row"], json.dumps(row), flush=True)
    for item in a.merge:
        name, path = item.split("=", 1)
        text = open(path).read()
        try:
            val = json.loads(text)
        except ValueError:
            val = [json.loads(l) for l in text.splitlines() if l.strip().startswith("{")]
        res.setdefault("unchanged_calls", {})[name] = val
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
