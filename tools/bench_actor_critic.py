"""What the value head in the rollout kernel and mev_gae cost against what a trainer does without them.

tools/bench_rollout.py's method: device pointers, one session, one device, a clock settle and a warm-up,
then per shape and rollout length T the time of blocks of calls by stream events, five blocks each,
alternating (median, min-max):
  values    (a) mev_rollout_policy_values: every *_seq output and value_seq
  rollout   (b) mev_rollout_policy on the same build and the same tensors
  eager_v   (c) what a user does today for the values: an eager torch forward (no_grad) of trunk + head over
            the (T + 1) E N rows of obs_0 and obs_seq
  gae       (d) mev_gae on the rollout's arrays (advantages, returns and valid, reset steps masked)
  eager_gae (e) the eager torch GAE loop over the same tensors: T iterations of elementwise kernels, the
            same recurrence and mask
The value path counts as a gain where (a) - (b) is below (c) by more than both blocks' spreads (the spread of
(a) - (b) taken as the sum of theirs); GAE likewise, (d) against (e).  Also recorded: VGPRs, spills and scratch
of every k_rollout instantiation and of k_gae from the code object, and -- given with --parent / --this, two
results of tools/bench_rollout.py --only cfg3_64 from the same session, one of the parent commit's build --
the comparison of the plain rollout before and after this change.
    python tools/bench_actor_critic.py [--out profiles/actor_critic_sweep.json] [--parent FILE --this FILE]"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_rollout as BR  # noqa: E402

SHAPES = [
    dict(name="cfg3_64", desc="4096 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2 + value head", E=4096, N=8,
         R=64, D=95, team=1, hidden=(64, 64), lengths=(16, 64)),
    dict(name="small", desc="64 envs x 8 agents x 64 beams, team reward, policy 95-64-64-2 + value head", E=64, N=8, R=64,
         D=95, team=1, hidden=(64, 64), lengths=(16, 64)),
]
RUNS, WARMUP, SETTLE_MS = BR.RUNS, BR.WARMUP, BR.SETTLE_MS
SUBSTEPS_PER_BLOCK = BR.SUBSTEPS_PER_BLOCK
GAMMA, LAM = 0.99, 0.95


def gae_resources(lib_path):
    """k_gae's line, with bench_rollout's reader pointed at it"""
    import subprocess
    import tempfile
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
    m = re.search(r"\.name:\s+(\S*k_gae\S*)\n", notes)
    if not m:
        return None
    s, e = notes.rfind(".agpr_count", 0, m.start()), notes.find(".agpr_count", m.end())
    blk = notes[s:e if e > 0 else None]
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
    return dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), vgpr_spills=get("vgpr_spill_count"),
                scratch_bytes=get("private_segment_fixed_size"))


def diff_stat(a, b, T):
    """(a) - (b) of two blocks' stats: the medians' difference, its spread the sum of theirs"""
    return dict(ms=round(a["ms"] - b["ms"], 5), spread=round(a["spread"] + b["spread"], 5),
                us_per_substep=round((a["ms"] - b["ms"]) * 1e3 / T, 3))


def verdict(ours_ms, ours_spread, theirs):
    m = max(ours_spread, theirs["spread"])
    return "gain" if theirs["ms"] - ours_ms > m else "loss" if ours_ms - theirs["ms"] > m else "tie"


def measure(cfg):
    import torch
    import pkgload
    mev = pkgload.load()
    dev = torch.device("cuda", 0)
    E, N, R, D = cfg["E"], cfg["N"], cfg["R"], cfg["D"]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=R, obs_dim=D, use_team_reward=cfg.get("team", 0),
                   max_steps=2000, seed=0, device=0)
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

    # trunk, actor and critic: weights ~ N(0, 1 / in), a positive throttle bias (the cars move)
    torch.manual_seed(7)
    nn = torch.nn
    dims = (D,) + tuple(cfg["hidden"])
    layers = []
    for i, o in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(i, o), nn.ReLU()]
    trunk, actor, critic = nn.Sequential(*layers).to(dev), nn.Linear(dims[-1], 2).to(dev), nn.Linear(dims[-1], 1).to(dev)
    with torch.no_grad():
        for lin in [m for m in trunk if isinstance(m, nn.Linear)] + [actor, critic]:
            lin.weight.normal_(0.0, lin.in_features ** -0.5)
            lin.bias.normal_(0.0, 0.1)
        actor.bias.copy_(torch.tensor([0.6, 0.0]))
    lins = [m for m in trunk if isinstance(m, nn.Linear)] + [actor]
    pol = h.policy([m.weight.detach() for m in lins], [m.bias.detach() for m in lins], device=True)
    pol.set_value_head(critic.weight.detach(), critic.bias.detach(), device=True)

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
        seqv = dict(seq, value_seq=z((T + 1, E, N), torch.float32))
        obs0 = z((E, N, D), torch.float32)
        ended_before = z((E,), torch.uint8)
        vals_eager = z((T + 1, E, N), torch.float32)
        gae_out = dict(advantages=z((T, E, N), torch.float32), returns=z((T, E, N), torch.float32), valid=z((T, E, N), torch.uint8))
        adv_e, ret_e, valid_e = z((T, E, N), torch.float32), z((T, E, N), torch.float32), z((T, E, N), torch.bool)

        def values_calls():
            for _ in range(calls):
                h.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seqv, device=True)

        def rollout_calls():
            for _ in range(calls):
                h.rollout_policy(pol, T, 1.0 / 60.0, auto_reset=True, out=seq, device=True)

        def eager_value_calls():
            with torch.no_grad():
                for _ in range(calls):
                    vals_eager[0] = critic(trunk(obs0.view(E * N, D))).view(E, N)
                    vals_eager[1:] = critic(trunk(seq["obs_seq"].view(T * E * N, D))).view(T, E, N)

        def gae_calls():
            for _ in range(calls):
                h.gae(seq["reward_seq"], seqv["value_seq"], seq["done_seq"], seq["terminated_seq"], seq["truncated_seq"],
                      ended_before, gamma=GAMMA, lam=LAM, mask_reset_steps=True, out=gae_out, device=True)

        def eager_gae_calls():
            r, V = seq["reward_seq"], seqv["value_seq"]
            with torch.no_grad():
                for _ in range(calls):
                    term, trunc = seq["terminated_seq"].bool(), seq["truncated_seq"].bool()
                    done = seq["done_seq"].bool()
                    ended = term | trunc
                    nxt = torch.zeros((E, N), device=dev)
                    for t in range(T - 1, -1, -1):
                        stop = done[t] | term[t][:, None]
                        cut = stop | trunc[t][:, None]
                        delta = r[t] + GAMMA * torch.where(stop, 0.0, V[t + 1]) - V[t]
                        adv = torch.where(cut, delta, delta + (GAMMA * LAM) * nxt)
                        before = (ended[t - 1] if t > 0 else ended_before.bool())[:, None]
                        adv = torch.where(before, 0.0, adv)
                        adv_e[t] = adv
                        valid_e[t] = ~before
                        nxt = adv
                    torch.add(adv_e, V[:T], out=ret_e)

        h.get_outputs(dict(obs=obs0), device=True)
        for fn in (values_calls, rollout_calls, eager_value_calls, gae_calls, eager_gae_calls):
            fn()  # warm every call of the timed blocks
        for fn in (values_calls, eager_value_calls, gae_calls, eager_gae_calls):
            fn()  # ... and once more from one window's arrays, for the check below
        torch.cuda.synchronize(dev)
        # the eager paths compute what the calls compute (not bit for bit: the framework's GEMM and FMA contraction)
        check = dict(values_max_abs_diff=float((vals_eager[1:] - seqv["value_seq"][1:]).abs().max()),
                     gae_max_abs_diff=float((adv_e - gae_out["advantages"]).abs().max()),
                     valid_equal=bool((valid_e == gae_out["valid"].bool()).all()))
        ta, tb, tc, td, te = [], [], [], [], []
        for _ in range(RUNS):
            ta.append(timed(values_calls) / calls)
            tb.append(timed(rollout_calls) / calls)
            tc.append(timed(eager_value_calls) / calls)
            td.append(timed(gae_calls) / calls)
            te.append(timed(eager_gae_calls) / calls)
        a, b, c, d, e = (BR.stat(v, T) for v in (ta, tb, tc, td, te))
        head = diff_stat(a, b, T)
        rows.append(dict(length=T, calls_per_block=calls, values=a, rollout=b, value_head_in_kernel=head, eager_values=c,
                         gae=d, eager_gae=e, value_verdict=verdict(head["ms"], head["spread"], c),
                         gae_verdict=verdict(d["ms"], d["spread"], e),
                         ratio_eager_values_over_head=round(c["ms"] / head["ms"], 3) if head["ms"] > 0 else None,
                         ratio_eager_gae_over_gae=round(e["ms"] / d["ms"], 3), check=check))
    res = dict(name=cfg["name"], workload=cfg["desc"], rollout_row=h.rollout_row(), runs=RUNS, clock_settle_steps=n_settle,
               warmup_steps=WARMUP, gamma=GAMMA, lam=LAM, rows=rows)
    pol.close()
    h.close()
    return res


def first_row(path):
    """row 0 (4096 x 8 x 64, 95-64-64-2, T = 16) of a tools/bench_rollout.py result"""
    with open(path) as f:
        r = json.load(f)
    shape = [s for s in r["shapes"] if s["name"] == "cfg3_64"][0]
    row = [x for x in shape["rows"] if x["length"] == 16][0]
    return row["rollout"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_critic_sweep.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--parent", default="", help="tools/bench_rollout.py --only cfg3_64 result of the parent commit's build")
    ap.add_argument("--this", default="", help="... of this build, from the same session")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_actor_critic.py needs a HIP device")
    import pkgload
    mev = pkgload.load()
    res = dict(method="stream events around blocks of 512 sub-steps' worth of calls, 5 alternated blocks each (median, "
                      "min-max), one process, one device; device pointers, auto-reset: (a) mev_rollout_policy_values, "
                      "(b) mev_rollout_policy, (c) eager torch trunk + head over the (T + 1) E N observation rows, "
                      "(d) mev_gae, (e) the eager torch GAE loop",
               device=torch.cuda.get_device_name(0), kernels=BR.kernel_resources(mev._capi.LIB_PATH),
               k_gae=gae_resources(mev._capi.LIB_PATH), shapes=[])
    for cfg in SHAPES:
        if a.only and a.only != cfg["name"]:
            continue
        r = measure(cfg)
        res["shapes"].append(r)
        for row in r["rows"]:
            print(r["name"], "row", r["rollout_row"], json.dumps(row), flush=True)
    if a.parent and a.this:
        p, t = first_row(a.parent), first_row(a.this)
        m = max(p["spread"], t["spread"])
        res["plain_rollout_parent_vs_this"] = dict(
            workload="tools/bench_rollout.py --only cfg3_64, T = 16: mev_rollout_policy, 4096 x 8 x 64, policy 95-64-64-2",
            parent=p, this=t, slower_by_ms=round(t["ms"] - p["ms"], 5), verdict="slower" if t["ms"] - p["ms"] > m else "not slower")
        print("plain rollout, parent vs this", json.dumps(res["plain_rollout_parent_vs_this"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
