"""What tanh activations cost inside the closed-loop rollout (MEV_POLICY_HIDDEN_TANH / MEV_POLICY_OUT_TANH), against
the loop a tanh user runs without them, and whether the ReLU calls kept the speed of the commit before.

Device pointers, auto-reset, every *_seq output, one session, one device, tools/bench_rollout.py's method: a clock
settle and a warm-up, then for each shape and rollout length T blocks of 512 sub-steps timed by stream events, five
blocks of each kind, alternating:
  tanh        (a)  mev_rollout_policy with a tanh-hidden policy
  tanh_out    (a') the same with the output tanh too
  eager       (b)  the loop a user runs today: per sub-step an eager torch forward of the same nn.Sequential(Linear,
                   Tanh, Linear, Tanh, Linear) (no_grad), a clamp into the action row and mev_step into the rows of
                   the same *_seq tensors
  relu        (c)  the ReLU policy of the same weights on this build
  relu_parent (d)  the ReLU policy on the library of the commit before (--parent-root: a checkout of it with its
                   library built, loaded into this process beside this build's, on a handle of its own)
and at the flagship shape the ReLU policy with a value head under mev_rollout_policy_repeat at n = 1, T = 16
(tools/bench_rollout_repeat.py's row), this build against the parent's, alternated the same way.
A shape counts as a gain only where (a) is below (b) by more than both blocks' spreads; a loss is reported as a loss.
The ReLU calls count as unchanged where (c) and (d) differ by no more than both blocks' spreads.  Also recorded: the
code-object figures of every k_rollout instantiation, and with --parent-root the parent's, matched by name.
    python tools/bench_rollout_act.py [--out profiles/rollout_act_sweep.json] [--only NAME] [--parent-root DIR]"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_rollout import RUNS, SETTLE_MS, SUBSTEPS_PER_BLOCK, WARMUP, kernel_resources, stat  # noqa: E402

SHAPES = [
    dict(name="cfg3_64", desc="4096 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2", E=4096, N=8, R=64, D=95,
         team=1, hidden=(64, 64), lengths=(16, 64), flagship=True),
    dict(name="small", desc="64 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2", E=64, N=8, R=64, D=95,
         team=1, hidden=(64, 64), lengths=(16,)),
]


def load_parent(root):
    """The package of a checkout of the commit before, under a name of its own; its library as it was built there."""
    pkg = os.path.join(root, "marl-traffic-intersection_amd")
    spec = importlib.util.spec_from_file_location("mev_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mev_parent"] = mod
    spec.loader.exec_module(mod)
    mod._capi._build.up_to_date = lambda variant="": True  # (never rebuilt here: the file that was handed in)
    mod.load_library()
    return mod


def verdict(a, b):
    """a against b: "faster" / "slower" only beyond both blocks' spreads"""
    d = a["ms"] - b["ms"]
    if abs(d) <= max(a["spread"], b["spread"]):
        return "tie"
    return "faster" if d < 0 else "slower"


def measure(cfg, mev, parent):
    import torch
    dev = torch.device("cuda", 0)
    E, N, R, D = cfg["E"], cfg["N"], cfg["R"], cfg["D"]
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    acts = torch.rand((4, E, N, 2), device=dev, generator=g) * 2.0 - 1.0

    def handle(pkg):
        h = pkg.Handle(num_envs=E, num_agents=N, lidar_rays=R, obs_dim=D, use_team_reward=cfg.get("team", 0),
                       max_steps=2000, seed=0, device=0)
        h.set_stream(st.cuda_stream)
        out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
        h.reset(device=True)
        return h, out

    h, out = handle(mev)
    hp, outp = handle(parent) if parent else (None, None)
    n_settle = 0
    t_end = time.perf_counter() + SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            h.step(acts[n_settle % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(WARMUP):
        h.step(acts[t % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
        if hp:
            hp.step(acts[t % 4].data_ptr(), 1.0 / 60.0, out=outp, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)

    # the policy: weights ~ N(0, 1 / in), a positive throttle bias (the cars move); one set of weights for all
    torch.manual_seed(7)
    nn = torch.nn
    dims = (D,) + tuple(cfg["hidden"]) + (2,)
    layers = []
    for i, o in zip(dims[:-1], dims[1:]):
        lin = nn.Linear(i, o)
        with torch.no_grad():
            lin.weight.normal_(0.0, i ** -0.5)
            lin.bias.normal_(0.0, 0.1)
        layers += [lin, nn.Tanh()]
    net = nn.Sequential(*layers[:-1]).to(dev)  # the module of (b): Linear, Tanh, Linear, Tanh, Linear
    with torch.no_grad():
        net[-1].bias.copy_(torch.tensor([0.6, 0.0]))
    lins = [m for m in net if isinstance(m, nn.Linear)]
    critic = nn.Linear(dims[-2], 1).to(dev)
    W, B = [m.weight.detach() for m in lins], [m.bias.detach() for m in lins]
    pols = dict(tanh=h.policy(W, B, device=True, hidden="tanh"), tanh_out=h.policy(W, B, device=True, hidden="tanh", out="tanh"),
                relu=h.policy(W, B, device=True))
    if hp:
        pols["relu_parent"] = hp.policy(W, B, device=True)
    owner = lambda k: hp if k == "relu_parent" else h
    lo_t, hi_t = torch.tensor([-1.0, -1.0], device=dev), torch.tensor([1.0, 1.0], device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    rows = []
    for T in cfg["lengths"]:
        calls = max(2, SUBSTEPS_PER_BLOCK // T)
        seq = dict(obs_seq=z((T, E, N, D), torch.float32), actions_seq=z((T, E, N, 2), torch.float32),
                   mean_seq=z((T, E, N, 2), torch.float32), reward_seq=z((T, E, N), torch.float32),
                   done_seq=z((T, E, N), torch.uint8), status_seq=z((T, E, N), torch.uint8),
                   terminated_seq=z((T, E), torch.uint8), truncated_seq=z((T, E), torch.uint8))
        step_out = [dict(obs=seq["obs_seq"][t], reward=seq["reward_seq"][t], done=seq["done_seq"][t],
                         status=seq["status_seq"][t], terminated=seq["terminated_seq"][t],
                         truncated=seq["truncated_seq"][t], agents_alive=out["agents_alive"], step=out["step"])
                    for t in range(T)]
        act_ptr = [seq["actions_seq"][t].data_ptr() for t in range(T)]
        first_obs = torch.zeros((E, N, D), dtype=torch.float32, device=dev)

        def rollout_calls(k):
            hh, pol = owner(k), pols[k]
            return lambda: [hh.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True) for _ in range(calls)]

        def eager_calls():
            with torch.no_grad():
                for _ in range(calls):
                    obs = first_obs
                    for t in range(T):
                        mu = net(obs.view(E * N, D))
                        torch.clamp(mu.view(E, N, 2), lo_t, hi_t, out=seq["actions_seq"][t])
                        h.step(act_ptr[t], 1.0 / 60.0, out=step_out[t], auto_reset=True, device=True)
                        obs = seq["obs_seq"][t]
                    first_obs.copy_(obs)  # (the next rollout's first observation: one copy per rollout, as a user keeps it)

        kinds = {k: rollout_calls(k) for k in pols}
        kinds["eager"] = eager_calls
        order = [k for k in ("tanh", "tanh_out", "eager", "relu", "relu_parent") if k in kinds]
        h.get_outputs(dict(obs=first_obs), device=True)
        for k in order:  # warm every call of the timed blocks
            kinds[k]()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in order}
        for _ in range(RUNS):
            for k in order:
                if k == "eager":
                    h.get_outputs(dict(obs=first_obs), device=True)
                times[k].append(timed(kinds[k]) / calls)
        s = {k: stat(v, T) for k, v in times.items()}
        a, b = s["tanh"], s["eager"]
        gain = b["min_max"][0] - a["min_max"][1] > 0 and b["ms"] - a["ms"] > max(a["spread"], b["spread"])
        loss = a["ms"] - b["ms"] > max(a["spread"], b["spread"])
        row = dict(length=T, rollouts_per_block=calls, **s, ratio_eager_over_tanh=round(b["ms"] / a["ms"], 4),
                   tanh_cost_us_per_substep=round((a["ms"] - s["relu"]["ms"]) * 1e3 / T, 3),
                   out_tanh_cost_us_per_substep=round((s["tanh_out"]["ms"] - a["ms"]) * 1e3 / T, 3),
                   verdict="gain" if gain else "loss" if loss else "tie")
        if hp:
            row["relu_against_parent"] = verdict(s["relu"], s["relu_parent"])
        rows.append(row)

    res = dict(name=cfg["name"], workload=cfg["desc"], rollout_row=h.rollout_row(), runs=RUNS,
               clock_settle_steps=n_settle, warmup_steps=WARMUP, rows=rows)

    if cfg.get("flagship"):  # the ReLU policy with a value head under mev_rollout_policy_repeat, n = 1, T = 16
        T = 16
        calls = SUBSTEPS_PER_BLOCK // T
        seq = dict(obs_seq=z((T, E, N, D), torch.float32), actions_seq=z((T, E, N, 2), torch.float32),
                   mean_seq=z((T, E, N, 2), torch.float32), reward_seq=z((T, E, N), torch.float32),
                   done_seq=z((T, E, N), torch.uint8), status_seq=z((T, E, N), torch.uint8),
                   terminated_seq=z((T, E), torch.uint8), truncated_seq=z((T, E), torch.uint8),
                   value_seq=z((T + 1, E, N), torch.float32), substeps_seq=z((T, E), torch.int32))
        kinds = {}
        for k in ("relu", "relu_parent") if hp else ("relu",):
            pols[k].set_value_head(critic.weight.detach().reshape(-1), critic.bias.detach(), device=True)
            kinds[k] = (lambda hh, pol: lambda: [hh.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True,
                                                                   repeat=1) for _ in range(calls)])(owner(k), pols[k])
        for k in kinds:
            kinds[k]()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in kinds}
        for _ in range(RUNS):
            for k in kinds:
                times[k].append(timed(kinds[k]) / calls)
        s = {k: stat(v, T) for k, v in times.items()}
        res["repeat_value_n1"] = dict(length=T, rollouts_per_block=calls, **s)
        if hp:
            res["repeat_value_n1"]["relu_against_parent"] = verdict(s["relu"], s["relu_parent"])

    for p in pols.values():
        p.close()
    h.close()
    if hp:
        hp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_act_sweep.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-root", default="", help="a checkout of the commit before, its library built: (d)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_act.py needs a HIP device")
    import pkgload
    mev = pkgload.load()
    mev.load_library()
    parent = load_parent(a.parent_root) if a.parent_root else None
    res = dict(method="stream events around blocks of 512 sub-steps (mev_rollout_policy with every *_seq output -- a tanh-hidden "
                      "policy, the same with the output tanh, the ReLU policy of the same weights on this build and on the "
                      "parent's library in the same process; an eager torch forward of the Tanh module, clamp and mev_step per "
                      "sub-step into the same tensors), 5 alternated blocks each (median, min-max), one process, one device; "
                      "device pointers, auto-reset",
               device=torch.cuda.get_device_name(0), kernels=kernel_resources(mev._capi.LIB_PATH), shapes=[])
    if parent:
        res["kernels_parent"] = kernel_resources(parent._capi.LIB_PATH)
        if res["kernels"] and res["kernels_parent"]:
            # (k_rollout has one more template flag here, ACT: the parent's instantiation is this build's with ACT = false)
            mine = lambda k: k + "ELb0" if "k_rollout" in k else k
            res["kernels_unchanged"] = all(res["kernels"].get(mine(k)) == v for k, v in res["kernels_parent"].items())
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg, mev, parent)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], "row", r["rollout_row"], json.dumps(row), flush=True)
        if "repeat_value_n1" in r:
            print(r["name"], "repeat, value head, n = 1", json.dumps(r["repeat_value_n1"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
