"""The C restatement (oracle/marl_oracle.c) against the reference itself at the edge poses: the
fixtures tests/golden/edge_<config>.npz hold pose sets of tests/edge_poses.py (grass edges, disc
rims, the screen border on both sides of pixel 0 and 750, boxes met exactly on their edge, twins
on both sides of the 1e-3 self-skip) written into the reference and stepped twice by it
(tests/golden/gen_golden.py, group `edge`).  An OracleEnv loaded with each recorded injected
state must reproduce both steps bit for bit: obs, reward, done, status, flags, ego and NPC state.

That the fixtures stand on the edges they are named for is counted from the recorded reference
data alone (never from the oracle), per fixture, and printed."""
import os

import numpy as np
import pytest

import edge_poses as EP
import golden_replay as G
import oracle_replay as ORP

F_NAMES = ["x", "y", "v", "h", "acc", "steer", "sx", "sy", "sv", "sh", "prev_dist", "pa0", "pa1"]
LARGEST_GOLDEN = "n12_r96_policy.npz"  # no fixture may be larger than the largest trajectory file


def routes_of(o, meta):
    L = int(meta["num_lanes"])
    rid = lambda se: o.route_id(G.point_index(se[0], L), G.point_index(se[1], L))  # noqa: E731
    return [rid(se) for se in meta["ego_routes"]], [rid(se) for se in meta["traffic_routes"]]


@pytest.mark.parametrize("name", EP.fixture_names())
def test_oracle_reproduces_the_reference_at_the_edge_poses(name):
    d = EP.load_fixture(name)
    meta = d["meta"]
    n, K = int(meta["n_agents"]), int(meta["npcs"])
    o = ORP.make_oracle(meta)
    ego_routes, tr = routes_of(o, meta)
    o.set_traffic_routes(tr)
    bad = []
    for p in range(int(meta["P"])):
        egos = ORP.state_from_records(d["init_ego_f"][p], d["init_ego_i"][p], ego_routes)
        npcs = ORP.state_from_records(d["init_npc_f"][p], d["init_npc_i"][p],
                                      [tr[r] for r in d["init_npc_i"][p][:, 3]]) if K else []
        o.set_state(egos, npcs, 0)
        for t in range(2):
            r = o.step(d["actions"][p, t], float(meta["dt"]), int(d["spawned"][p, t]) if meta["traffic"] else -1)
            tag = f"pose set {p} ({EP.KINDS[int(d['kind'][p])]}) step {t + 1}"
            errs = []
            if not G.bits_equal(r["obs"][:, :127], d["obs"][p, t]):
                w = np.argwhere(r["obs"][:, :127].view(np.uint32) != d["obs"][p, t].view(np.uint32))
                errs.append(f"obs at (agent, col) {w[:6].tolist()}")
            if "lidar" in d and not G.bits_equal(r["obs"][:, 31:], d["lidar"][p, t] * np.float32(1.0 / meta["max_dist"])):
                errs.append("full lidar")
            if not G.bits_equal(r["rew"], d["rew"][p, t]):
                errs.append("reward")
            if not G.bits_equal(r["done"], d["done"][p, t]) or not G.bits_equal(r["status"], d["status"][p, t]):
                errs.append(f"status {r['status'].tolist()} vs {d['status'][p, t].tolist()}")
            if [r["terminated"], r["truncated"], r["agents_alive"], r["step"]] != [int(v) for v in d["flags"][p, t]]:
                errs.append("flags")
            egos_o, npcs_o, _ = o.get_state()
            for j, nm in enumerate(F_NAMES):
                if not G.bits_equal(egos_o[nm], d["ego_f"][p, t][:, j]):
                    errs.append(f"ego {nm}")
            if not (G.bits_equal(egos_o["len"], d["ego_f"][p, t][:, 13]) and G.bits_equal(egos_o["wid"], d["ego_f"][p, t][:, 14])):
                errs.append("ego length / width")
            for j, nm in enumerate(["alive", "intention", "path_index"]):
                if not np.array_equal(egos_o[nm], d["ego_i"][p, t][:, j]):
                    errs.append(f"ego {nm}")
            kc = int(d["npc_count"][p, t])
            if len(npcs_o) != kc:
                errs.append(f"npc count {len(npcs_o)} vs {kc}")
            else:
                for j, nm in enumerate(F_NAMES[:6]):
                    if not G.bits_equal(npcs_o[nm], d["npc_f"][p, t][:kc, j]):
                        errs.append(f"npc {nm}")
                if not np.array_equal(npcs_o["path_index"], d["npc_i"][p, t][:kc, 2]):
                    errs.append("npc path_index")
            if errs:
                bad.append(f"{tag}: {'; '.join(errs)}")
                break
    o.close()
    assert not bad, f"{len(bad)} pose sets differ from the reference:\n" + "\n".join(bad[:10])


def f32(v):
    return np.asarray(v, np.float32)


def counts(d):
    """What the recorded reference data shows of the edges, from step 1 (the LiDAR of the state after it)."""
    meta = d["meta"]
    n, K, R, P = int(meta["n_agents"]), int(meta["npcs"]), int(meta["rays"]), int(meta["P"])
    fov, maxd = float(meta["fov"]), float(meta["max_dist"])
    slots = min(R, 96)
    kind = d["kind"]
    lid = d["obs"][:, 0, :, 31:31 + slots]  # [P][n][slots]
    ef = d["ego_f"][:, 0]  # [P][n][15] after step 1
    stopped = (lid > 0) & (lid < 1.0)
    quad = EP.beam_quadrants(ef[:, :, 3], R, fov)[..., :slots]
    edge = np.isin(kind, EP.EDGE_KINDS)
    out = dict(stopped=int(stopped.sum()), quadrants=sorted(q for q in range(4) if (stopped[edge] & (quad[edge] == q)).any()))
    # border: a centre in (-1, 0) whose pixel int() makes 0 -- on screen, so beams run on and stop
    # on grass (floor() would make it -1: every beam broken off at once, none stopped)
    neg = ((ef[:, :, 0] > -1) & (ef[:, :, 0] < 0)) | ((ef[:, :, 1] > -1) & (ef[:, :, 1] < 0))
    out["border_neg_pixel0"] = int((neg & (kind == 4)[:, None] & stopped.any(-1)).sum())
    # the pairs of the box and twin kinds: (ego 2k, ego 2k + 1), or (the ego, NPC 0); standing pose sets only
    first = f32(meta["lidar_step"]) * f32(1.0 / maxd)  # a beam stopped by the first probe past the centre
    probes = EP.probe_distances(maxd, float(meta["lidar_step"]))
    rel0 = f32(-fov) * f32(0.5) * f32(np.pi) / f32(180.0)
    out.update(twins_hidden=0, twins_hidden_far_beam=0, twins_seen=0, box_on_edge=0, box_hits=0)
    for p in np.flatnonzero((np.arange(P) % 2 == 0) & np.isin(kind, (5, 6))):
        pairs = [(ef[p, i], ef[p, i + 1], lid[p, i], lid[p, i + 1]) for i in range(0, n - 1, 2)]
        if n == 1 and K and int(d["npc_count"][p, 0]) and \
                np.abs(d["npc_f"][p, 0, 0, :2] - d["init_npc_f"][p, 0, :2]).max() < 1.0:  # (NPC 0 is still there)
            pairs = [(ef[p, 0], d["npc_f"][p, 0, 0], lid[p, 0], None)]
        for a, b, la, lb in pairs:
            if kind[p] == 6:
                hidden = all(np.abs(f32(b[c]) - f32(a[c])) < f32(1e-3) for c in (0, 1, 3))  # Lidar.cpp:59-61
                blocks = [la] + ([lb] if lb is not None else [])
                if hidden:
                    out["twins_hidden"] += 1
                    out["twins_hidden_far_beam"] += int(all((l_ > first).any() for l_ in blocks))
                else:  # each stands inside the other's box: every beam stops at the first probe
                    out["twins_seen"] += 1
                    assert all((l_ == first).all() for l_ in blocks), f"pose set {p}: a visible twin left a beam free"
            else:
                k = np.flatnonzero(probes * f32(1.0 / maxd) == la[0])
                ang = float(f32(a[3]) + rel0)
                dx, dy = np.cos(ang), -np.sin(ang)
                if len(k) != 1 or max(abs(dx), abs(dy)) < 1 - 1e-6:
                    continue
                c = 0 if abs(dx) > abs(dy) else 1  # the axis beam 0 runs along: its component is exactly +-1
                sgn = f32(np.round(dx if c == 0 else dy))
                px = f32(int(f32(a[c]) + sgn * probes[k[0]]))  # Lidar.cpp:34-35
                hl, hw = f32(b[13]) * f32(0.5), f32(b[14]) * f32(0.5)
                ca, sa = np.abs(np.cos(f32(b[3]))), np.abs(np.sin(f32(b[3])))
                ext = (ca * hl + sa * hw, sa * hl + ca * hw)[c]  # Lidar.cpp:71-72
                out["box_hits"] += 1
                out["box_on_edge"] += int(px == f32(b[c]) - f32(ext) or px == f32(b[c]) + f32(ext))
    return out


@pytest.mark.parametrize("name", EP.fixture_names())
def test_fixture_stands_on_the_edges(name):
    d = EP.load_fixture(name)
    P = int(d["meta"]["P"])
    assert P >= 64 and P % 16 == 0 and P == EP.FIXTURES[name]["P"]
    size = os.path.getsize(os.path.join(EP.GOLDEN_DIR, f"edge_{name}.npz"))
    assert size <= os.path.getsize(os.path.join(EP.GOLDEN_DIR, LARGEST_GOLDEN)), size
    assert int((d["spawned"] >= 0).sum()) == 0  # deterministic: no spawns
    c = counts(d)
    print(f"edge_{name}: {size // 1024} KB, P={P}, {c}")
    assert c["stopped"] > 0 and c["quadrants"] == [0, 1, 2, 3], c
    assert c["border_neg_pixel0"] >= 1, c
    assert c["twins_seen"] >= 1 and c["twins_hidden"] >= 1 and c["twins_hidden_far_beam"] >= 1, c
    assert c["box_on_edge"] >= 1, c
