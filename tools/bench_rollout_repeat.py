"""What frame skip inside a closed-loop rollout (mev_rollout_policy_repeat) costs against what a user runs without it.

tools/bench_rollout.py's method: device pointers, auto-reset, every *_seq output, a clock settle and a warm-up as
bench.py does, then for each shape the time of CALLS rollouts of T decisions x n sub-steps by stream events, five
blocks each, alternating:
  repeat    (a) mev_rollout_policy_repeat with every *_seq output, value_seq and substeps_seq
  eager     (b) the same semantics without it: per decision an eager torch forward pass of trunk and value head
            (no_grad) on the previous observation row, a clamp into the preallocated action row, and mev_step_repeat
            (auto-reset) into the rows of the same tensors -- all on the handle's stream
  substeps  (c) mev_rollout_policy_values over T * n sub-steps: a new action every sub-step and nothing summed --
            other semantics, for orientation only
A shape counts as a gain only where (a) is below (b) by more than both blocks' spreads; a loss is reported as one.
Also recorded: the VGPRs, spills, scratch and static LDS of every k_rollout instantiation and of the flagship k_step
row from the library's code object and, with --parent-lib, from the library of the commit before, matched by
template arguments (the REPEAT flag is a new last argument); and, with --merge NAME=FILE, other runs' JSON (the
unchanged calls timed on both builds in the same session) under "unchanged_calls".
    python tools/bench_rollout_repeat.py [--out profiles/rollout_repeat_sweep.json] [--only NAME] [--parent-lib SO]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIG = dict(E=4096, N=8, R=64, D=95, team=1, hidden=(64, 64), T=16)
SHAPES = [
    dict(BIG, name="cfg3_64", desc="4096 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2 with a value head",
         repeats=(1, 2, 4, 8)),
    dict(BIG, name="small", desc="64 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2 with a value head", E=64,
         repeats=(4,)),
    dict(BIG, name="cfg4", desc="4096 envs x 1 agent x 64 beams, traffic density 0.5, policy 95-64-64-2 with a value head",
         N=1, team=0, traffic=1, repeats=(4,)),
    dict(BIG, name="cfg3_64_runtime_row", desc="4096 envs x 8 agents x 64 beams, one car 55 x 24 (per-car sizes: the "
         "runtime-layout row), policy 95-64-64-2 with a value head", dims=1, repeats=(4,)),
]
RUNS, WARMUP, SETTLE_MS = 5, 100, 200.0
SUBSTEPS_PER_BLOCK = 512  # CALLS = SUBSTEPS_PER_BLOCK / (T n) rollouts per timed block


def med(v):
    return sorted(v)[len(v) // 2]


def stat(v, T, n):
    return dict(ms=round(med(v), 5), min_max=[round(min(v), 5), round(max(v), 5)], spread=round(max(v) - min(v), 5),
                us_per_decision=round(med(v) * 1e3 / T, 3), us_per_substep=round(med(v) * 1e3 / (T * n), 3))


def kernel_resources(lib_path):
    """Every k_rollout instantiation and k_step's flagship row from the code object's metadata, keyed by template
    arguments; None without the LLVM tools."""
    llvm = "/opt/rocm/llvm/bin"
    try:
        with tempfile.TemporaryDirectory() as d:
            fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
            subprocess.run([f"{llvm}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib_path, os.path.join(d, "x")],
                           check=True, capture_output=True)
            subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", f"--input={fat}", "--unbundle",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    except Exception:
        return None
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n", notes):
        # the mangled name's template arguments: Lb0E / Lb1E a bool, Li<n>E an int
        t = re.match(r"_ZN3mev\d+(k_rollout|k_step)I((?:L[bi]\d+E)+)E", m.group(1))
        if not t:
            continue
        args = [v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([bi])(\d+)E", t.group(2))]
        if t.group(1) == "k_rollout":
            args = args + ["false"] * (9 - len(args))  # (a build before REPEAT: seven arguments; before MULTI: eight)
            key = "k_rollout<" + ", ".join(args[:7]) + ">" + (" REPEAT" if args[7] == "true" else "") + \
                (" MULTI" if args[8] == "true" else "")
        elif len(args) == 10 and args[:3] == ["false", "false", "8"] and args[7:] == ["64", "8", "true"]:
            key = "k_step<" + ", ".join(args) + "> (8 x 64, the world at compile time: the flagship row)"
        else:
            continue
        s, e = notes.rfind(".agpr_count", 0, m.start()), notes.find(".agpr_count", m.end())
        blk = notes[s:e if e > 0 else None]
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        res[key] = dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), vgpr_spills=get("vgpr_spill_count"),
                        sgpr_spills=get("sgpr_spill_count"), scratch_bytes=get("private_segment_fixed_size"),
                        static_lds_bytes=get("group_segment_fixed_size"))
    return res


def measure(cfg):
    import numpy as np
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R, D, T = cfg["E"], cfg["N"], cfg["R"], cfg["D"], cfg["T"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, obs_dim=D, use_team_reward=cfg.get("team", 0),
                   traffic_flow=cfg.get("traffic", 0), traffic_density=0.5, max_steps=2000, seed=0, device=0)
    if cfg.get("dims"):
        ego = np.tile(np.array([54.0, 24.0], np.float32), (E, N, 1))
        ego[0, 0, 0] = 55.0
        h.set_car_dims(ego, None)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    h.set_stream(st.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    acts = torch.rand((4, E, N, 2), device=dev, generator=g) * 2.0 - 1.0
    out = {k: torch.zeros_like(torch.as_tensor(v), device=dev) for k, v in h.alloc_outputs().items()}
    h.reset(device=True)
    n_settle = 0
    t_end = time.perf_counter() + SETTLE_MS * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(64):
            h.step(acts[n_settle % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
            n_settle += 1
        torch.cuda.synchronize(dev)
    for t in range(WARMUP):
        h.step(acts[t % 4].data_ptr(), 1.0 / 60.0, out=out, auto_reset=True, device=True)
    torch.cuda.synchronize(dev)

    # the policy: weights ~ N(0, 1 / in), a positive throttle bias (the cars move), and a value head on the trunk
    torch.manual_seed(7)
    nn = torch.nn
    dims = (D,) + tuple(cfg["hidden"]) + (2,)
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
    lo_t, hi_t = torch.tensor([-1.0, -1.0], device=dev), torch.tensor([1.0, 1.0], device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)

    def seqs(rows):
        return dict(obs_seq=z((rows, E, N, D), torch.float32), actions_seq=z((rows, E, N, 2), torch.float32),
                    mean_seq=z((rows, E, N, 2), torch.float32), reward_seq=z((rows, E, N), torch.float32),
                    done_seq=z((rows, E, N), torch.uint8), status_seq=z((rows, E, N), torch.uint8),
                    terminated_seq=z((rows, E), torch.uint8), truncated_seq=z((rows, E), torch.uint8),
                    value_seq=z((rows + 1, E, N), torch.float32))

    rows = []
    for n in cfg["repeats"]:
        calls = max(2, SUBSTEPS_PER_BLOCK // (T * n))
        seq = dict(seqs(T), substeps_seq=z((T, E), torch.int32))
        sub = seqs(T * n)  # (c)'s rows: one per sub-step
        step_out = [dict(obs=seq["obs_seq"][t], reward=seq["reward_seq"][t], done=seq["done_seq"][t],
                         status=seq["status_seq"][t], terminated=seq["terminated_seq"][t],
                         truncated=seq["truncated_seq"][t], agents_alive=out["agents_alive"], step=out["step"],
                         substeps=seq["substeps_seq"][t]) for t in range(T)]
        act_ptr = [seq["actions_seq"][t].data_ptr() for t in range(T)]
        first_obs = torch.zeros((E, N, D), dtype=torch.float32, device=dev)

        def repeat_calls():
            for _ in range(calls):
                h.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True, repeat=n)

        def eager_calls():
            with torch.no_grad():
                for _ in range(calls):
                    obs = first_obs
                    for t in range(T):
                        hid = trunk(obs.view(E * N, D))
                        seq["value_seq"][t].copy_(critic(hid).view(E, N))
                        torch.clamp(actor(hid).view(E, N, 2), lo_t, hi_t, out=seq["actions_seq"][t])
                        h.step_repeat(act_ptr[t], n, 1.0 / 60.0, out=step_out[t], auto_reset=True, device=True)
                        obs = seq["obs_seq"][t]
                    seq["value_seq"][T].copy_(critic(trunk(obs.view(E * N, D))).view(E, N))
                    first_obs.copy_(obs)  # (the next rollout's first observation: one copy per rollout, as a user keeps it)

        def substep_calls():
            for _ in range(calls):
                h.rollout_policy(pol, T * n, 1.0 / 60.0, auto_reset=True, out=sub, device=True)

        h.get_outputs(dict(obs=first_obs), device=True)
        repeat_calls(), eager_calls(), substep_calls()  # warm every call of the timed blocks
        torch.cuda.synchronize(dev)
        ta, tb, tc = [], [], []
        for _ in range(RUNS):
            ta.append(timed(repeat_calls) / calls)
            h.get_outputs(dict(obs=first_obs), device=True)
            tb.append(timed(eager_calls) / calls)
            tc.append(timed(substep_calls) / calls)
        a, b, c = stat(ta, T, n), stat(tb, T, n), stat(tc, T, n)
        gain = b["min_max"][0] - a["min_max"][1] > 0 and b["ms"] - a["ms"] > max(a["spread"], b["spread"])
        loss = a["ms"] - b["ms"] > max(a["spread"], b["spread"])
        rows.append(dict(decisions=T, repeat=n, rollouts_per_block=calls, repeat_call=a, eager=b, every_substep=c,
                         ratio_eager_over_repeat=round(b["ms"] / a["ms"], 4),
                         mean_substeps=round(float(seq["substeps_seq"].float().mean()), 3),
                         verdict="gain" if gain else "loss" if loss else "tie"))
    res = dict(name=cfg["name"], workload=cfg["desc"], rollout_row=h.rollout_row(), runs=RUNS,
               clock_settle_steps=n_settle, warmup_steps=WARMUP, rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    pol.close()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_repeat_sweep.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-lib", default="", help="the library built from the commit before: its register figures")
    ap.add_argument("--merge", action="append", default=[], metavar="NAME=FILE",
                    help="another run's JSON (or JSON-lines) output, stored under unchanged_calls[NAME]")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_repeat.py needs a HIP device")
    import pkgload
    mev = pkgload.load()
    res = dict(method="stream events around blocks of 512 sub-steps (mev_rollout_policy_repeat with every *_seq output, "
                      "value_seq and substeps_seq; an eager torch forward of trunk, actor and value head, a clamp and "
                      "mev_step_repeat per decision into the same tensors; mev_rollout_policy_values over T n "
                      "sub-steps), 5 alternated blocks each (median, min-max), one process, one device; device "
                      "pointers, auto-reset",
               device=torch.cuda.get_device_name(0), kernels=kernel_resources(mev._capi.LIB_PATH), shapes=[])
    if a.parent_lib:
        res["kernels_parent"] = kernel_resources(a.parent_lib)
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
