"""The frame-skip contract (mev_step_repeat, include/marlenv.h) as a loop over the oracle.

`repeat_step` is the reference's driver loop (test.py:144-155) over one OracleEnv: the same
action for up to `repeat` steps, the reward summed in f32 in step order, done / status latched
at each agent's latest done, stopping at terminated or truncated.  `RepeatRef` runs it for
every env of a batch with the vector env's auto-reset (reset() before the window of an env
whose previous window ended) and counts what the windows covered, so that a test can assert
that its scenario reached the cases it is about."""
import numpy as np

import oracle_replay as R

ROUTES3 = [(1, 4), (2, 8), (3, 12), (4, 7), (5, 11), (6, 3), (7, 10), (8, 2), (9, 6), (10, 1), (11, 5), (12, 9)]
REWARD = [10.0, 1.0, -0.01, -10.0, -5.0, 10.0, -0.02, 0.2]
CRASH_WALL, CRASH_LINE, CRASH_CAR = 3, 4, 5


def repeat_step(o, a, dt, repeat, spawn=None):
    """One frame-skip window of OracleEnv o.  spawn: the `repeat` traffic-route indices of the
    sub-steps (None: no spawn attempts).  Returns the window's outputs (the keys of
    OracleEnv.step plus substeps) and, under "sub", every executed sub-step's own result."""
    acc = any_done = latched = None
    sub = []
    for s in range(repeat):
        r = o.step(a, dt, -1 if spawn is None else int(spawn[s]))
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


def meta(N, rays, use_team=False, respawn=True, max_steps=2000, traffic=False, density=0.5):
    return dict(rays=rays, obs_dim=127, num_lanes=3, n_agents=N, use_team=use_team, respawn=respawn,
                max_steps=max_steps, traffic=traffic, density=density, reward=REWARD)


def ego_routes(route_id, E, N):
    """Agent i of env e on the (e + i) % 12-th default 3-lane route; route_id(start, end) -> id."""
    ids = [route_id(s - 1, 12 + t - 1) for s, t in ROUTES3]
    return np.array([[ids[(e + i) % 12] for i in range(N)] for e in range(E)], np.int32), ids


def draw(rng, E, N, bias, repeat=0, traffic=False):
    """One call's inputs, in the draw order the tests share."""
    a = rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)
    a[..., 0] += bias
    sp = rng.integers(-1, 12, (repeat, E)) if traffic else None
    return a, sp


class RepeatRef:
    """E oracle envs stepped in frame-skip windows with per-env auto-reset."""

    def __init__(self, oracles, routes):
        self.oracles = list(oracles)
        self.routes = np.asarray(routes)
        self.ended = [False] * len(self.oracles)
        self.mid_dones = self.early_stops = self.resets = self.peak_npcs = 0
        self.status_count = {CRASH_WALL: 0, CRASH_LINE: 0, CRASH_CAR: 0}
        self.early_k = []

    def step(self, a, dt, repeat, sp=None, auto_reset=True):
        out = []
        for e, o in enumerate(self.oracles):
            if auto_reset and self.ended[e]:
                o.reset([int(r) for r in self.routes[e]])
                self.resets += 1
            w = repeat_step(o, a[e], dt, repeat, None if sp is None else sp[:, e])
            k = w["substeps"]
            for s, r in enumerate(w["sub"]):
                last = s == k - 1
                for c in self.status_count:
                    self.status_count[c] += int(((r["done"] != 0) & (r["status"] == c)).sum())
                # a done in a sub-step that is neither the window's last nor the env's end
                # (dead agents, done at every step, do not count)
                if not last and ((r["done"] != 0) & (r["status"] >= 2)).any():
                    self.mid_dones += 1
            if k < repeat:
                self.early_stops += 1
                self.early_k.append(k)
            self.ended[e] = bool(w["terminated"] or w["truncated"])
            out.append(w)
        return out

    def close(self):
        for o in self.oracles:
            o.close()


def check_window(tag, out, e, w):
    """Every output of env e of a device frame-skip call equals the window w, bit for bit."""
    R.check_step(tag, out, e, w)
    assert int(out["substeps"][e]) == w["substeps"], tag + ": substeps"
