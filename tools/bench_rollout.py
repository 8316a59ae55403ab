"""What a closed-loop rollout in one launch (mev_rollout_policy) costs against the loop a user runs without it.

Device pointers, one session, one device, tools/bench_evaluate.py's method: a clock settle and a warm-up
as bench.py does, then for each shape and rollout length T the time of CALLS rollouts by stream events,
five blocks each, alternating:
  rollout   (a) mev_rollout_policy with every *_seq output
  eager     (b) the same trajectory without it: per sub-step an eager torch nn.Sequential forward pass
            (no_grad) on the previous observation row, a clamp into the preallocated action row, and
            mev_step (auto-reset) into the rows of the same *_seq tensors -- all on the handle's stream
  steps     (c) T x mev_step alone on ready-made action rows: the floor; (a) - (c) is the policy's cost
            inside the kernel
A shape counts as a gain only where (a) is below (b) by more than both blocks' spreads.  Also recorded:
the kernels' VGPRs, spills, scratch and static LDS from the library's code object (when the LLVM tools
are there), and at 4096 x 8 x 64 the runtime-layout row against the compile-time row: the same batch
with one car one pixel longer (mev_set_car_dims), which the compile-time layout cannot run.
    python tools/bench_rollout.py [--out profiles/rollout_sweep.json] [--only NAME]"""
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

SHAPES = [
    dict(name="cfg3_64", desc="4096 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2", E=4096, N=8, R=64, D=95,
         team=1, hidden=(64, 64), lengths=(16, 64)),
    dict(name="cfg3_128", desc="4096 envs x 8 agents x 64 beams, team reward, policy 95-128-128-2", E=4096, N=8, R=64,
         D=95, team=1, hidden=(128, 128), lengths=(16, 64)),
    dict(name="cfg3_64_runtime_row", desc="4096 envs x 8 agents x 64 beams, one car 55 x 24 (per-car sizes: the "
         "runtime-layout row at the compile-time row's shape), policy 95-64-64-2", E=4096, N=8, R=64, D=95, team=1,
         dims=1, hidden=(64, 64), lengths=(16,)),
    dict(name="cfg4", desc="4096 envs x 1 agent x 64 beams, traffic density 0.5, policy 95-64-64-2", E=4096, N=1, R=64,
         D=95, traffic=1, hidden=(64, 64), lengths=(16,)),
    dict(name="small", desc="64 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2", E=64, N=8, R=64, D=95,
         team=1, hidden=(64, 64), lengths=(16,)),
]
RUNS, WARMUP, SETTLE_MS = 5, 100, 200.0
SUBSTEPS_PER_BLOCK = 512  # CALLS = SUBSTEPS_PER_BLOCK / T rollouts per timed block
SEQS = ("obs_seq", "actions_seq", "mean_seq", "reward_seq", "done_seq", "status_seq", "terminated_seq", "truncated_seq")


def med(v):
    return sorted(v)[len(v) // 2]


def stat(v, T):
    return dict(ms=round(med(v), 5), min_max=[round(min(v), 5), round(max(v), 5)], spread=round(max(v) - min(v), 5),
                us_per_substep=round(med(v) * 1e3 / T, 3))


def kernel_resources(lib_path):
    """k_rollout's rows (and the flagship k_step) from the code object's metadata, or None without the tools."""
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
        name = m.group(1)
        if "k_rollout" not in name and "k_policy_repack" not in name:
            continue
        s, e = notes.rfind(".agpr_count", 0, m.start()), notes.find(".agpr_count", m.end())
        blk = notes[s:e if e > 0 else None]
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        key = re.sub(r"^_ZN3mev\d+|EEEv.*$", "", name)
        res[key] = dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), vgpr_spills=get("vgpr_spill_count"),
                        sgpr_spills=get("sgpr_spill_count"), scratch_bytes=get("private_segment_fixed_size"),
                        static_lds_bytes=get("group_segment_fixed_size"))
    return res


def measure(cfg):
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R, D = cfg["E"], cfg["N"], cfg["R"], cfg["D"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, obs_dim=D, use_team_reward=cfg.get("team", 0),
                   traffic_flow=cfg.get("traffic", 0), traffic_density=0.5, max_steps=2000, seed=0, device=0)
    if cfg.get("dims"):
        import numpy as np
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
    step_row = h.step_row()

    # the policy: weights ~ N(0, 1 / in), a positive throttle bias (the cars move)
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
    net = nn.Sequential(*layers[:-1]).to(dev)
    with torch.no_grad():
        net[-1].bias.copy_(torch.tensor([0.6, 0.0]))
    lins = [m for m in net if isinstance(m, nn.Linear)]
    pol = h.policy([m.weight.detach() for m in lins], [m.bias.detach() for m in lins], device=True)
    lo_t, hi_t = torch.tensor([-1.0, -1.0], device=dev), torch.tensor([1.0, 1.0], device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    rows = []
    for T in cfg["lengths"]:
        calls = max(2, SUBSTEPS_PER_BLOCK // T)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        seq = dict(obs_seq=z((T, E, N, D), torch.float32), actions_seq=z((T, E, N, 2), torch.float32),
                   mean_seq=z((T, E, N, 2), torch.float32), reward_seq=z((T, E, N), torch.float32),
                   done_seq=z((T, E, N), torch.uint8), status_seq=z((T, E, N), torch.uint8),
                   terminated_seq=z((T, E), torch.uint8), truncated_seq=z((T, E), torch.uint8))
        # the per-sub-step output dicts of (b) and (c): row t of the same tensors
        step_out = [dict(obs=seq["obs_seq"][t], reward=seq["reward_seq"][t], done=seq["done_seq"][t],
                         status=seq["status_seq"][t], terminated=seq["terminated_seq"][t],
                         truncated=seq["truncated_seq"][t], agents_alive=out["agents_alive"], step=out["step"])
                    for t in range(T)]
        act_ptr = [seq["actions_seq"][t].data_ptr() for t in range(T)]
        first_obs = torch.zeros((E, N, D), dtype=torch.float32, device=dev)

        def rollout_calls():
            for _ in range(calls):
                h.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True)

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

        def step_calls():
            for _ in range(calls):
                for t in range(T):
                    h.step(act_ptr[t], 1.0 / 60.0, out=step_out[t], auto_reset=True, device=True)

        h.get_outputs(dict(obs=first_obs), device=True)
        rollout_calls(), eager_calls(), step_calls()  # warm every call of the timed blocks
        torch.cuda.synchronize(dev)
        t_roll, t_eager, t_step = [], [], []
        for _ in range(RUNS):
            t_roll.append(timed(rollout_calls) / calls)
            h.get_outputs(dict(obs=first_obs), device=True)
            t_eager.append(timed(eager_calls) / calls)
            t_step.append(timed(step_calls) / calls)
        a, b, c = stat(t_roll, T), stat(t_eager, T), stat(t_step, T)
        gain = b["min_max"][0] - a["min_max"][1] > 0 and b["ms"] - a["ms"] > max(a["spread"], b["spread"])
        loss = a["ms"] - b["ms"] > max(a["spread"], b["spread"])
        rows.append(dict(length=T, rollouts_per_block=calls, rollout=a, eager=b, steps=c,
                         ratio_eager_over_rollout=round(b["ms"] / a["ms"], 4),
                         policy_in_kernel_us_per_substep=round((a["ms"] - c["ms"]) * 1e3 / T, 3),
                         verdict="gain" if gain else "loss" if loss else "tie"))
    res = dict(name=cfg["name"], workload=cfg["desc"], rollout_row=h.rollout_row(), step_row=step_row,
               runs=RUNS, clock_settle_steps=n_settle, warmup_steps=WARMUP, rows=rows)
    if cfg.get("traffic"):
        res["mean_npcs"] = round(float(h.get_state()["npc_count"].mean()), 2)
    pol.close()
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_sweep.json"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout.py needs a HIP device")
    import pkgload
    mev = pkgload.load()
    res = dict(method="stream events around blocks of 512 sub-steps (mev_rollout_policy with every *_seq output; an eager "
                      "torch nn.Sequential forward, clamp and mev_step per sub-step into the same tensors; mev_step alone "
                      "on ready-made actions), 5 alternated blocks each (median, min-max), one process, one device; "
                      "device pointers, auto-reset",
               device=torch.cuda.get_device_name(0), kernels=kernel_resources(mev._capi.LIB_PATH), shapes=[])
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], "row", r["rollout_row"], json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
