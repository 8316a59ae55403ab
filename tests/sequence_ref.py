"""The plan-rollout contract (mev_step_sequence, include/marlenv.h) as a loop over the oracle.

`sequence_step` steps one OracleEnv through a plan: sub-step s takes its own action A[s], its own
dt and spawn decision, the reward is summed in f32 in step order, done / status are latched at
each agent's latest done, and the env stops at its first terminated or truncated sub-step.
`SequenceRef` runs it for every env of a batch with the vector env's auto-reset (modelled on
repeat_ref.RepeatRef) and counts what the windows covered, so that a test can assert that its
scenario reached the cases it is about."""
import numpy as np

import golden_replay as G
import oracle_replay as R
from repeat_ref import CRASH_CAR, CRASH_LINE, CRASH_WALL

DT = 1.0 / 60.0


def sequence_step(o, A, dts, spawn=None):
    """One plan of OracleEnv o: A [T][N][2], dts [T], spawn [T] traffic-route indices (None: no
    spawn attempts).  Returns the call's outputs (the keys of OracleEnv.step plus substeps)
    and, under "sub", every executed sub-step's own result."""
    acc = any_done = latched = None
    sub = []
    for s in range(len(A)):
        r = o.step(A[s], float(dts[s]), -1 if spawn is None else int(spawn[s]))
        sub.append(r)
        if s == 0:
            acc = r["rew"].astype(np.float32).copy()
            any_done = np.zeros_like(r["done"])
            latched = np.zeros_like(r["status"])
        else:
            acc = (acc + r["rew"]).astype(np.float32)  # f32, in sub-step order
        d = r["done"] != 0
        any_done[d] = 1
        latched[d] = r["status"][d]
        if r["terminated"] or r["truncated"]:
            break
    r = sub[-1]
    return dict(obs=r["obs"], rew=acc, done=any_done, status=np.where(any_done != 0, latched, r["status"]),
                terminated=r["terminated"], truncated=r["truncated"], agents_alive=r["agents_alive"],
                step=r["step"], substeps=len(sub), sub=sub)


def draw(rng, E, N, T, bias, traffic=False):
    """One call's inputs, in the draw order the tests share: a per-call base action every sub-step
    varies around (uncorrelated per-step actions average out and hardly crash)."""
    base = rng.uniform(-1, 1, (E, N, 2))
    A = (base[None] + 0.25 * rng.uniform(-1, 1, (T, E, N, 2))).astype(np.float32)
    A[..., 0] += np.float32(bias)
    dts = rng.choice([DT, DT / 2, 1.5 * DT], T).astype(np.float32)
    sp = rng.integers(-1, 12, (T, E)) if traffic else None
    return A, dts, sp


class SequenceRef:
    """E oracle envs stepped through plans with per-env auto-reset."""

    def __init__(self, oracles, routes):
        self.oracles = list(oracles)
        self.routes = np.asarray(routes)
        self.ended = [False] * len(self.oracles)
        self.mid_dones = self.early_stops = self.resets = self.peak_npcs = 0
        self.status_count = {CRASH_WALL: 0, CRASH_LINE: 0, CRASH_CAR: 0}
        self.early_k = []

    def step(self, A, dts, sp=None, auto_reset=True):
        T = len(A)
        out = []
        for e, o in enumerate(self.oracles):
            if auto_reset and self.ended[e]:
                o.reset([int(r) for r in self.routes[e]])
                self.resets += 1
            w = sequence_step(o, A[:, e], dts, None if sp is None else sp[:, e])
            k = w["substeps"]
            for s, r in enumerate(w["sub"]):
                last = s == k - 1
                for c in self.status_count:
                    self.status_count[c] += int(((r["done"] != 0) & (r["status"] == c)).sum())
                # a done in a sub-step that is neither the window's last nor the env's end
                # (dead agents, done at every step, do not count)
                if not last and ((r["done"] != 0) & (r["status"] >= 2)).any():
                    self.mid_dones += 1
            if k < T:
                self.early_stops += 1
                self.early_k.append(k)
            self.ended[e] = bool(w["terminated"] or w["truncated"])
            out.append(w)
        return out

    def close(self):
        for o in self.oracles:
            o.close()


def check_plan(tag, out, e, w, T):
    """Every output of env e of a device plan rollout equals the oracle's window w, bit for bit:
    the final outputs, the sub-step count, each executed sub-step's own row, all-zero bits in the
    rows after the env stopped, and reward == the sequential f32 sum of its rows."""
    R.check_step(tag, out, e, w)
    k = w["substeps"]
    assert int(out["substeps"][e]) == k, tag + ": substeps"
    rs, ds, ss = out["reward_seq"], out["done_seq"], out["status_seq"]
    assert rs.shape[0] == ds.shape[0] == ss.shape[0] == T, tag + ": rows"
    for s, r in enumerate(w["sub"]):
        assert G.bits_equal(rs[s, e], r["rew"]), f"{tag}: reward_seq row {s}"
        assert G.bits_equal(ds[s, e], r["done"]), f"{tag}: done_seq row {s}"
        assert G.bits_equal(ss[s, e], r["status"]), f"{tag}: status_seq row {s}"
    assert not rs[k:, e].view(np.uint32).any(), tag + ": reward_seq rows after the stop are not zero bits"
    assert not ds[k:, e].any() and not ss[k:, e].any(), tag + ": done_seq / status_seq rows after the stop"
    acc = rs[0, e].copy()
    for s in range(1, T):
        acc = (acc + rs[s, e]).astype(np.float32)
    assert G.bits_equal(acc, out["reward"][e]), tag + ": reward is not the sequential f32 sum of its rows"
