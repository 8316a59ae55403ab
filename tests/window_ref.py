"""The window contract (mev_step_repeat and mev_step_sequence, include/marlenv.h) as a loop over
the oracle, and the scenario helpers the GPU tests of both calls share.

`window_step` steps one OracleEnv through up to T sub-steps as the reference's driver loops its
step (test.py:144-155): sub-step s takes the action A[s], its own dt and spawn decision, the
reward is summed in f32 in step order, done / status are latched at each agent's latest done, and
the env stops at its first terminated or truncated sub-step.  Frame skip is the window whose rows
are one held action (`held`); a plan rollout has a row of its own per sub-step.  `WindowRef` runs
it for every env of a batch with the vector env's auto-reset (reset() before the window of an env
whose previous window ended) and counts what the windows covered, so that a test can assert that
its scenario reached the cases it is about."""
import numpy as np

import golden_replay as G
import oracle_replay as R

ROUTES3 = [(1, 4), (2, 8), (3, 12), (4, 7), (5, 11), (6, 3), (7, 10), (8, 2), (9, 6), (10, 1), (11, 5), (12, 9)]
REWARD = [10.0, 1.0, -0.01, -10.0, -5.0, 10.0, -0.02, 0.2]
CRASH_WALL, CRASH_LINE, CRASH_CAR = 3, 4, 5
DT = 1.0 / 60.0
OUT_KEYS = ("obs", "reward", "done", "status", "terminated", "truncated", "agents_alive", "step")


def window_step(o, A, dts, spawn=None):
    """One window of OracleEnv o: A [T][N][2], dts [T], spawn [T] traffic-route indices (None: no
    spawn attempts).  Returns the call's outputs (the keys of OracleEnv.step plus substeps)
    and, under "sub", every executed sub-step's own result."""
    acc = any_done = latched = None
    sub = []
    for s in range(len(A)):
        r = o.step(A[s], dts[s], -1 if spawn is None else int(spawn[s]))
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


def held(a, dt, n):
    """The rows (A, dts) of a frame-skip window: the action a and dt in each of n sub-steps."""
    return np.broadcast_to(a, (n,) + np.shape(a)), [dt] * n


def meta(N, rays, use_team=False, respawn=True, max_steps=2000, traffic=False, density=0.5):
    return dict(rays=rays, obs_dim=127, num_lanes=3, n_agents=N, use_team=use_team, respawn=respawn,
                max_steps=max_steps, traffic=traffic, density=density, reward=REWARD)


def ego_routes(route_id, E, N):
    """Agent i of env e on the (e + i) % 12-th default 3-lane route; route_id(start, end) -> id."""
    ids = [route_id(s - 1, 12 + t - 1) for s, t in ROUTES3]
    return np.array([[ids[(e + i) % 12] for i in range(N)] for e in range(E)], np.int32), ids


def draw(rng, E, N, bias, repeat=0, traffic=False):
    """One frame-skip call's inputs, in the draw order the tests share."""
    a = rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)
    a[..., 0] += bias
    sp = rng.integers(-1, 12, (repeat, E)) if traffic else None
    return a, sp


def draw_plan(rng, E, N, T, bias, traffic=False):
    """One plan's inputs, in the draw order the tests share: a per-call base action every sub-step
    varies around (uncorrelated per-step actions average out and hardly crash)."""
    base = rng.uniform(-1, 1, (E, N, 2))
    A = (base[None] + 0.25 * rng.uniform(-1, 1, (T, E, N, 2))).astype(np.float32)
    A[..., 0] += np.float32(bias)
    dts = rng.choice([DT, DT / 2, 1.5 * DT], T).astype(np.float32)
    sp = rng.integers(-1, 12, (T, E)) if traffic else None
    return A, dts, sp


class WindowRef:
    """E oracle envs stepped in windows with per-env auto-reset."""

    def __init__(self, oracles, routes):
        self.oracles = list(oracles)
        self.routes = np.asarray(routes)
        self.ended = [False] * len(self.oracles)
        self.mid_dones = self.early_stops = self.resets = self.peak_npcs = 0
        self.status_count = {CRASH_WALL: 0, CRASH_LINE: 0, CRASH_CAR: 0}
        self.early_k = []

    def step(self, A, dts, sp=None, auto_reset=True):
        """A [T][E][N][2], dts [T], sp [T][E] or None -> each env's window_step result."""
        T = len(A)
        out = []
        for e, o in enumerate(self.oracles):
            if auto_reset and self.ended[e]:
                o.reset([int(r) for r in self.routes[e]])
                self.resets += 1
            w = window_step(o, A[:, e], dts, None if sp is None else sp[:, e])
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


def check_window(tag, out, e, w, T=None):
    """Every output of env e of a device window call equals the oracle's window w, bit for bit: the
    final outputs and the sub-step count; for a plan of T rows also each executed sub-step's own
    row, all-zero bits in the rows after the env stopped, and reward == the sequential f32 sum of
    its rows."""
    R.check_step(tag, out, e, w)
    k = w["substeps"]
    assert int(out["substeps"][e]) == k, tag + ": substeps"
    if T is None:
        return
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


# ---- the GPU tests' scenario: a handle, its oracles, and calls checked against them ----------------

def handle(mev, E, N, rays, use_team=False, respawn=True, max_steps=2000, traffic=False, density=0.5, max_npcs=32,
           seed=7):
    return mev.Handle(num_envs=E, num_agents=N, lidar_rays=rays, obs_dim=127, use_team_reward=int(use_team),
                      respawn_enabled=int(respawn), max_steps=max_steps, traffic_flow=int(traffic),
                      traffic_density=density, max_npcs=max_npcs, seed=seed, device=0)


def set_routes(h, traffic=False):
    """The tests' ego routes (and, with traffic, NPC routes) on handle h, then a reset."""
    routes, ids = ego_routes(h.route_id, h.E, h.N)
    h.set_ego_routes(routes)
    if traffic:
        h.set_traffic_routes(ids)
    h.reset()
    return routes, ids


def start(h, meta, traffic=False):
    """Routes, reset, and the oracles of a handle's envs in the same state."""
    routes, ids = set_routes(h, traffic)
    oracles = []
    for e in range(h.E):
        o = R.make_oracle(meta)
        if traffic:
            o.set_traffic_routes(ids)
        o.reset([int(r) for r in routes[e]])
        oracles.append(o)
    return WindowRef(oracles, routes)


def scenario(mev, E, N, rays, n, calls, seed, bias, plan, prepare=None, traffic=False, max_npcs=32, dims=False, **cfg):
    """`calls` windows of n sub-steps -- frame skip, or with `plan` plan rollouts -- on a new handle
    (prepare(h): further setup of it) against its oracles: every output and the full state after
    every call.  Returns the WindowRef with its coverage counters."""
    h = handle(mev, E, N, rays, traffic=traffic, max_npcs=max_npcs, **cfg)
    if prepare:
        prepare(h)
    ref = start(h, meta(N, rays, traffic=traffic, **cfg), traffic)
    if dims:  # per-car sizes, the same on both sides (an auto-reset gives new cars of 54 x 24 again)
        drng = np.random.default_rng(40)
        ego = np.stack([drng.uniform(40, 70, (E, N)), drng.uniform(18, 30, (E, N))], -1).astype(np.float32)
        h.set_car_dims(ego, None)
        for e, o in enumerate(ref.oracles):
            egos, npcs, sc = o.get_state()
            egos["len"], egos["wid"] = ego[e, :, 0], ego[e, :, 1]
            o.set_state(egos, npcs, sc)
    rng = np.random.default_rng(seed)
    for c in range(calls):
        if plan:
            A, dts, sp = draw_plan(rng, E, N, n, bias, traffic)
            out = h.step_sequence(A, dts, spawn_route=sp, auto_reset=True)
        else:
            a, sp = draw(rng, E, N, bias, n, traffic)
            out = h.step_repeat(a, n, DT, spawn_route=sp, auto_reset=True)
            A, dts = held(a, DT, n)
        ws = ref.step(A, dts, sp)
        st = h.get_state()
        cd = h.car_dims() if dims else None
        for e in range(E):
            check_window(f"call {c} env {e}", out, e, ws[e], n if plan else None)
            R.check_state(f"call {c} env {e}", st, e, ref.oracles[e], cd)
        if traffic:
            ref.peak_npcs = max(ref.peak_npcs, max(len(o.get_state()[1]) for o in ref.oracles))
    h.close()
    ref.close()
    return ref
