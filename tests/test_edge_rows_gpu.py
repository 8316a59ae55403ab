"""Every compiled step kernel at the edge poses.  One case per entry of tests/step_rows.py (every row
of kStepKeys and kServeKeys, with and without the distance table) and one per fixture
configuration on the two-kernel path (k_cars + k_lidar).  A case creates the entry's handle,
asserts that Handle.step_row() is the entry's row (so a change of the plan that moves the shape to
another kernel fails here instead of silently testing that one twice), places cars at the poses of
tests/edge_poses.py (all seven kinds, interleaved by env; with traffic also seven NPCs), steps once
with zero actions and respawn off, and compares every output and the state after the step bit for
bit with the C restatement (oracle/marl_oracle.c) per env.  Step entries run launched (the
persistent server off), serve entries must be answered by the server.  Where the entry's
configuration is a fixture's (tests/golden/edge_<config>.npz, recorded from the reference itself),
the fixture's pose sets are stepped too and compared with the recorded reference outputs
directly, both steps.

The window calls' leaf casts are other LiDAR instantiations than the step's: from the same poses,
step_sequence (T = 1), step_repeat (n = 1) and evaluate_plans(leaf_obs) (T = 1, one candidate per
env) must give the step's obs / reward / done / status bit for bit, at three shapes.

Nothing here places cars to make a kernel fault: poses stay within [-30, 780]."""
import numpy as np
import pytest

import edge_poses as EP
import golden_replay as G
import oracle_replay as ORP
import step_rows as SR

pytestmark = pytest.mark.gpu

NPCS = 7  # NPCs placed beside the ego of a traffic entry
BATCHES = 2
DEFAULT_REWARD = [10.0, 1.0, -0.01, -10.0, -5.0, 10.0, -0.02, 0.2]
# the two-kernel path at each fixture's configuration
PATH1 = [dict(SR.DEFAULTS, table="path1", row=-1, tab=int(f["lidar_step"] != 4.0), name=f"path1_{name}", kernel=1,
              max_npcs=32, **{k: f[k] for k in EP.CONFIG_KEYS})
         for name, f in EP.FIXTURES.items()]
CASES = SR.ENTRIES + PATH1


def make_handle(mev, e, monkeypatch):
    """The entry's handle, its scheduling calls made and its row asserted."""
    if e["no_world_const"]:
        monkeypatch.setenv("MEV_NO_WORLD_CONST", "1")
    else:
        monkeypatch.delenv("MEV_NO_WORLD_CONST", raising=False)
    h = mev.Handle(**SR.config(e))
    if e["kernel"]:
        h.set_step_kernel(e["kernel"])
    if e["pack"]:
        h.set_step_pack(e["pack"])
    if e["split"]:
        h.set_step_split(e["split"])
    if not e["serve"]:
        h.set_serve(0)
    set_dims(h, e)
    row = h.step_row()
    if e["table"] == "step":
        assert (row["step"], row["tab"]) == (e["row"], e["tab"]), (e["name"], row)
    elif e["table"] == "serve":
        assert (row["serve"], row["tab"]) == (e["row"], e["tab"]), (e["name"], row)
    else:
        assert (row["step"], row["tab"]) == (-1, e["tab"]) and h.step_kernel() == 1, (e["name"], row)
    return h


def set_dims(h, e, ego=None):
    if e["dims"]:
        d = np.asarray(EP.EGO_DIMS, np.float32)[np.arange(h.N) % len(EP.EGO_DIMS)] if ego is None else ego
        h.set_car_dims(ego=np.broadcast_to(d, (h.E, h.N, 2)))


def oracle_meta(e, D):
    return dict(num_lanes=e["lanes"], n_agents=e["n"], rays=e["rays"], obs_dim=D, use_team=False, respawn=False,
                max_steps=2000, traffic=bool(e["traffic"]), density=0.0, reward=DEFAULT_REWARD, fov=e["fov"],
                max_dist=e["max_dist"], lidar_step=e["lidar_step"])


def load_oracle(o, st, b, n, dims):
    """Env b of a device state (mev_get_state arrays, Handle.car_dims()) into oracle o."""
    cars = ORP.O.new_cars(n)
    for a, f in ORP.EGO_FIELDS.items():
        cars[a] = st[f][b]
    k = int(st["npc_count"][b])
    npcs = ORP.O.new_cars(k)
    for a, f in ORP.NPC_FIELDS.items():
        npcs[a] = st[f][b, :k]
    if dims is not None:
        cars["len"], cars["wid"] = dims[0][b, :, 0], dims[0][b, :, 1]
        npcs["len"], npcs["wid"] = dims[1][b, :k, 0], dims[1][b, :k, 1]
    o.set_state(cars, npcs, int(st["step_count"][b]))


def place(h, e, rng, troutes):
    """A batch of edge poses into handle h (standing cars; with traffic NPCS NPCs per env); the state as the device holds it."""
    n, K = h.N, NPCS if e["traffic"] else 0
    dims = EP.EGO_DIMS if e["dims"] else None
    x, y, hd = EP.poses(rng, n + K, E=h.E, num_lanes=e["lanes"], kinds=len(EP.KINDS), fov=e["fov"],
                        lidar_step=e["lidar_step"], dims=dims, npcs=K)
    st = h.get_state()
    st["x"][:], st["y"][:], st["heading"][:] = x[:, :n], y[:, :n], hd[:, :n]
    st["alive"][:] = 1
    for f in ("v", "acc", "steering"):
        st[f][:] = 0.0
    if K:
        st["npc_count"][:] = K
        st["npc_x"][:, :K], st["npc_y"][:, :K], st["npc_heading"][:, :K] = x[:, n:], y[:, n:], hd[:, n:]
        for f in ("npc_v", "npc_acc", "npc_steering"):
            st[f][:, :K] = 0.0
        st["npc_path_index"][:, :K] = rng.integers(0, 150, (h.E, K))
        st["npc_route"][:, :K] = np.asarray(troutes)[rng.integers(0, len(troutes), (h.E, K))]
        st["npc_intention"][:, :K] = 0
        st["npc_alive"][:, :K] = 1
    h.set_state(st)
    set_dims(h, e)
    return h.get_state()


def step_checked(h, e, acts, spawn):
    """One host-mode step; a serve entry's must be answered by the server, any other's launched."""
    s0 = h.serve_stats()["steps"]
    out = h.step(acts, spawn_route=spawn)
    assert h.serve_stats()["steps"] - s0 == (1 if e["serve"] else 0), (e["name"], h.serve_stats())
    return out


def run_oracle_batches(h, e, seed):
    n, R, D = h.N, h.R, h.D
    rng = np.random.default_rng(seed)
    troutes = h.default_traffic_routes() if e["traffic"] else None
    o = ORP.make_oracle(oracle_meta(e, D))
    if e["traffic"]:
        o.set_traffic_routes([int(r) for r in troutes])
    slots = min(R, D - 31)
    stops, quads = 0, set()
    acts = np.zeros((h.E, n, 2), np.float32)
    spawn = np.full(h.E, -1, np.int32) if e["traffic"] else None
    for _ in range(BATCHES):
        st = place(h, e, rng, troutes)
        dims = h.car_dims() if e["dims"] else None
        out = step_checked(h, e, acts, spawn)
        gst = h.get_state()
        gdims = h.car_dims() if e["dims"] else None
        want = np.zeros((h.E, n, slots), np.float32)
        for b in range(h.E):
            load_oracle(o, st, b, n, dims)
            r = o.step(acts[b], 1.0 / 60.0, -1)
            tag = f"{e['name']} env {b} ({EP.KINDS[b % len(EP.KINDS)]})"
            if not G.bits_equal(out["obs"][b], r["obs"]):
                bad = np.argwhere(out["obs"][b].view(np.uint32) != r["obs"].view(np.uint32))
                i, c = bad[0]
                raise AssertionError(
                    f"{tag}: {len(bad)} obs words differ, first agent {i} col {c}: got {out['obs'][b][i, c]!r} want "
                    f"{r['obs'][i, c]!r}; pose {float(st['x'][b, i])!r}, {float(st['y'][b, i])!r}, "
                    f"{float(st['heading'][b, i])!r}; differing (agent, col): {bad[:12].tolist()}")
            ORP.check_step(tag, out, b, r)
            ORP.check_state(tag, gst, b, o, gdims)
            want[b] = r["obs"][:, 31:31 + slots]
        # not vacuous (from the oracle's rows): beams stopped, and from the edge kinds in every direction quadrant
        stopped = (want > 0) & (want < 1.0)
        quad = EP.beam_quadrants(gst["heading"], R, e["fov"])[..., :slots]
        edge = np.isin(np.arange(h.E) % len(EP.KINDS), EP.EDGE_KINDS)
        stops += int(stopped.sum())
        quads |= {q for q in range(4) if (stopped[edge] & (quad[edge] == q)).any()}
    o.close()
    assert stops > 0
    assert quads == {0, 1, 2, 3}, quads


def run_fixture(h, e, name):
    """The fixture's recorded pose sets through handle h, E at a time: both steps against the recorded reference."""
    d = EP.load_fixture(name)
    meta = d["meta"]
    n, K, L, D = h.N, int(meta["npcs"]), int(meta["num_lanes"]), h.D
    rid = lambda se: h.route_id(G.point_index(se[0], L), G.point_index(se[1], L))  # noqa: E731
    ego_routes = [rid(se) for se in meta["ego_routes"]]
    troutes = [rid(se) for se in meta["traffic_routes"]]
    if e["traffic"]:
        h.set_traffic_routes(troutes)
    W = min(D, 127)
    P = int(meta["P"])
    for p0 in range(0, P, h.E):
        ps = [min(p0 + b, P - 1) for b in range(h.E)]  # (a short last batch repeats its last pose set)
        st = h.get_state()
        for j, key in enumerate(G.EGO_F):
            st[key][:] = d["init_ego_f"][ps][:, :, j]
        ii = d["init_ego_i"][ps]
        st["alive"][:], st["intention"][:], st["path_index"][:], st["route"][:] = ii[..., 0], ii[..., 1], ii[..., 2], ego_routes
        st["step_count"][:] = 0
        st["npc_count"][:] = K
        if K:
            nf, ni = d["init_npc_f"][ps], d["init_npc_i"][ps]
            for j, key in enumerate(G.NPC_F):
                st[key][:, :K] = nf[:, :, j]
            st["npc_alive"][:, :K], st["npc_intention"][:, :K], st["npc_path_index"][:, :K] = ni[..., 0], ni[..., 1], ni[..., 2]
            st["npc_route"][:, :K] = np.asarray(troutes)[ni[..., 3]]
        h.set_state(st)
        set_dims(h, e, d["init_ego_f"][ps][:, :, 13:15])
        for t in range(2):
            acts = np.ascontiguousarray(d["actions"][ps, t])
            spawn = np.ascontiguousarray(d["spawned"][ps, t]) if e["traffic"] else None
            out = step_checked(h, e, acts, spawn)
            gst = h.get_state()
            for b, p in enumerate(ps):
                tag = f"{e['name']} fixture {name} pose set {p} ({EP.KINDS[int(d['kind'][p])]}) step {t + 1}"
                got = out["obs"][b]
                if not G.bits_equal(got[:, :W], d["obs"][p, t][:, :W]):
                    bad = np.argwhere(got[:, :W].view(np.uint32) != d["obs"][p, t][:, :W].view(np.uint32))
                    raise AssertionError(f"{tag}: obs differs from the reference at (agent, col) {bad[:12].tolist()}")
                if "lidar" in d and D >= 31 + h.R:
                    assert G.bits_equal(got[:, 31:31 + h.R], d["lidar"][p, t] * np.float32(1.0 / e["max_dist"])), tag + ": lidar"
                assert G.bits_equal(out["reward"][b], d["rew"][p, t]), tag + ": reward"
                assert G.bits_equal(out["done"][b], d["done"][p, t]) and G.bits_equal(out["status"][b], d["status"][p, t]), \
                    tag + ": done / status"
                flags = [int(out["terminated"][b]), int(out["truncated"][b]), int(out["agents_alive"][b]), int(out["step"][b])]
                assert flags == [int(v) for v in d["flags"][p, t]], tag + ": flags"
                ef, ei = d["ego_f"][p, t], d["ego_i"][p, t]
                for j, key in enumerate(G.EGO_F):
                    assert G.bits_equal(gst[key][b], ef[:, j]), f"{tag}: ego {key}"
                assert G.bits_equal(gst["alive"][b], ei[:, 0].astype(np.uint8)) and G.bits_equal(gst["intention"][b], ei[:, 1]) \
                    and G.bits_equal(gst["path_index"][b], ei[:, 2]), tag + ": ego alive / intention / path_index"
                kc = int(d["npc_count"][p, t])
                assert int(gst["npc_count"][b]) == kc, tag + ": npc count"
                for j, key in enumerate(G.NPC_F):
                    assert G.bits_equal(gst[key][b, :kc], d["npc_f"][p, t][:kc, j]), f"{tag}: {key}"
                assert G.bits_equal(gst["npc_path_index"][b, :kc], d["npc_i"][p, t][:kc, 2]), tag + ": npc path_index"


@pytest.mark.parametrize("entry", CASES, ids=[e["name"] for e in CASES])
def test_row_at_the_edge_poses(mev, entry, monkeypatch):
    h = make_handle(mev, entry, monkeypatch)
    try:
        run_oracle_batches(h, entry, 1000 + CASES.index(entry))
        name = EP.fixture_for(entry)
        if name is not None:
            run_fixture(h, entry, name)
        assert entry["table"] != "path1" or name is not None
    finally:
        h.close()


WINDOW_SHAPES = [dict(SR.DEFAULTS, name="8x64", kernel=0), dict(SR.DEFAULTS, name="1x64_pack4", n=1, pack=4),
                 dict(SR.DEFAULTS, name="traffic_1x64_k32", n=1, traffic=1, kernel=0)]


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=[s["name"] for s in WINDOW_SHAPES])
def test_window_calls_match_the_step_at_the_edge_poses(mev, shape, monkeypatch):
    e = dict(shape, table="window", row=-1, tab=0)
    monkeypatch.delenv("MEV_NO_WORLD_CONST", raising=False)
    h = mev.Handle(**SR.config(e))
    try:
        if e["kernel"]:
            h.set_step_kernel(e["kernel"])
        if e["pack"]:
            h.set_step_pack(e["pack"])
        h.set_serve(0)
        E, n = h.E, h.N
        rng = np.random.default_rng(77 + WINDOW_SHAPES.index(shape))
        place(h, e, rng, h.default_traffic_routes() if e["traffic"] else None)
        acts = np.zeros((E, n, 2), np.float32)
        sp = (lambda *s: np.full(s, -1, np.int32)) if e["traffic"] else (lambda *s: None)
        # (evaluate_plans leaves the handle as it is; the others start from a snapshot of the placed batch)
        ev = h.evaluate_plans(acts[None], np.arange(E, dtype=np.int32), leaf_obs=True, spawn_route=sp(1, E))
        snap = h.snapshot()
        want = {k: v.copy() for k, v in h.step(acts, spawn_route=sp(E)).items()}
        assert ((want["obs"][:, :, 31:] > 0) & (want["obs"][:, :, 31:] < 1.0)).any()
        h.restore(snap)
        seq = h.step_sequence(acts[None], spawn_route=sp(1, E))
        h.restore(snap)
        rep = h.step_repeat(acts, 1, spawn_route=sp(1, E))
        for tag, got in (("step_sequence", seq), ("step_repeat", rep)):
            for k in ("obs", "reward", "done", "status"):
                assert G.bits_equal(got[k], want[k]), f"{shape['name']}: {tag} {k} differs from the step's"
            assert (got["substeps"] == 1).all()
        assert G.bits_equal(ev["leaf_obs"], want["obs"]), f"{shape['name']}: evaluate_plans leaf_obs differs from the step's obs"
        assert G.bits_equal(ev["reward_seq"][0], want["reward"]), "evaluate_plans reward"
        assert G.bits_equal(ev["done_seq"][0], want["done"]) and G.bits_equal(ev["status_seq"][0], want["status"]), \
            "evaluate_plans done / status"
    finally:
        h.close()
