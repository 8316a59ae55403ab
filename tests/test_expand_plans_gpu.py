"""State pools and mev_expand_plans (include/marlenv.h): plan evaluations whose candidates may start
from a slot of a device pool and whose stop states are kept in one.  A stored slot (Pool.get_state,
car sizes included) is checked bit for bit against the oracle that ran the candidate's window from
its root's device state (window_ref.window_step), every shared output against mev_evaluate_plans /
mev_evaluate_leaves on the same inputs, and a chain of two expansions through a slot against the
single call with the concatenated plan.  Every output buffer is filled with 0xFF bytes before a
call.  The scenarios, histories, plans and helpers are those of tests/test_evaluate_plans_gpu.py
and tests/test_evaluate_leaves_gpu.py, imported.

Chosen on the CPU with the oracle alone (the history replayed by oracles): scenario PLAIN's stops are
truncations, so its sub-step counts are [1, 1, 1, 5, 5, 3, 1, 5, 5, 5, 1, 3, 5] for every plan seed;
with plan seed 47 no candidate crashes in the sub-step it stops at, with plan seed 64 candidates 5
(truncated at its third sub-step) and 12 (at the plan's last) do, so this file draws its plans with
64.  Split 2 + 3, 8 candidates go on from their slots: 6 run through, 2 stop inside the second part."""
import numpy as np
import pytest

import golden_replay as G
import oracle_replay as R
import test_evaluate_leaves_gpu as EL
import test_evaluate_plans_gpu as EP
import window_ref as RR
from test_evaluate_plans_gpu import ALL, PLAIN, ROOTS13, SEQ, TRAFFIC, TWELVE
from window_ref import CRASH_WALL, DT

pytestmark = pytest.mark.gpu

PLAN_SEED = 64
KS = [1, 1, 1, 5, 5, 3, 1, 5, 5, 5, 1, 3, 5]
OUT = ALL + ("leaf_obs",)


# ---- helpers ----

def windows(meta, state, roots, A, dts, sp=None, traffic_routes=None, dims=None):
    """Each candidate's window from an oracle holding its root's state; the oracles stay open, in the
    state the candidate stopped at (the caller closes them)."""
    ws, os_ = [], []
    for c, r in enumerate(roots):
        o = R.oracle_from_device_state(meta, state, int(r), traffic_routes, dims)
        ws.append(RR.window_step(o, A[:, c], dts, None if sp is None else sp[:, c]))
        os_.append(o)
    return ws, os_


def close_all(os_):
    for o in os_:
        o.close()


def expand(h, A, roots, dts, gamma, dst, dst_slots, src=None, off=0, sp=None, leaf=True):
    T, C = A.shape[0], A.shape[1]
    return h.expand_plans(A, roots, dst, dst_slots, src, off, leaf, dts, gamma, spawn_route=sp,
                          out=EL.outputs(T, C, h.N, h.D if leaf else None))


def check_slots(tag, pool, slots, os_):
    """The slots against the oracles' states, car sizes included; all valid."""
    st, dims, valid = pool.get_state(slots)
    assert valid.tolist() == [1] * len(slots), tag + ": valid bytes"
    for i, o in enumerate(os_):
        R.check_state(f"{tag}: slot {slots[i]}", st, i, o, dims)


def same_slots(tag, pool, a, b):
    """Slots a and b hold the same states: every ego field, the live NPC prefix, counters, sizes."""
    (sa, da, va), (sb, db, vb) = pool.get_state(a), pool.get_state(b)
    assert va.all() and vb.all(), tag + ": valid bytes"
    assert G.bits_equal(sa["npc_count"], sb["npc_count"]) and G.bits_equal(sa["step_count"], sb["step_count"]), tag
    assert G.bits_equal(da[0], db[0]), tag + ": ego sizes"
    for i, k in enumerate(sa["npc_count"]):
        assert G.bits_equal(da[1][i, :k], db[1][i, :k]), f"{tag}: NPC sizes of pair {i}"
    for name in sa:
        if not name.startswith("npc_"):
            assert G.bits_equal(sa[name], sb[name]), f"{tag}: {name}"
        elif name != "npc_count":
            for i, k in enumerate(sa["npc_count"]):
                assert G.bits_equal(sa[name][i, :k], sb[name][i, :k]), f"{tag}: {name} of pair {i}"


def crash_at_stop(ws):
    """candidates with a crash (respawn on: a respawn) in the sub-step they stop at"""
    return [c for c, w in enumerate(ws)
            if ((w["sub"][-1]["done"] != 0) & (w["sub"][-1]["status"] >= CRASH_WALL)).any()]


def check_tail(tag, full, tail, cs, t1):
    """The second call's outputs for candidates cs against rows t1.. of the single call."""
    for c in cs:
        for k in SEQ:
            assert G.bits_equal(tail[k][:, c], full[k][t1:, c]), f"{tag}: {k} of candidate {c}"
        assert int(tail["substeps"][c]) == int(full["substeps"][c]) - t1, f"{tag}: substeps of candidate {c}"
        for k in ("terminated", "truncated", "leaf_obs"):
            if k in tail:
                assert G.bits_equal(tail[k][c], full[k][c]), f"{tag}: {k} of candidate {c}"


# ---- scenario 1 (shared: computed once, never changed).  One pool: slots [0, 13) the single call's
# stop states, [13, 26) the first part's (2 sub-steps), [26, 39) the second part's (3, from [13, 26)),
# the rest never written ----

@pytest.fixture(scope="module")
def plain(mev):
    P = PLAIN
    h, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
    EP._device_history_plain(h, P["seed"])
    before = EP._snap_all(h)
    C = len(ROOTS13)
    A, dts = EP.plans_plain(np.random.default_rng(PLAN_SEED), P["N"], ROOTS13, P["T"])
    pool = h.pool(48)
    assert pool.slots == 48 and not pool.get_state(np.arange(48))[2].any()  # (valid bytes start at 0)
    slots = np.arange(C, dtype=np.int32)
    full = expand(h, A, ROOTS13, dts, P["gamma"], pool, slots)
    leaf, scored = EL.both(h, A, ROOTS13, dts, P["gamma"])
    first = expand(h, A[:2], ROOTS13, dts[:2], P["gamma"], pool, slots + C)
    second = expand(h, A[2:], slots + C, dts[2:], P["gamma"], pool, slots + 2 * C, src=pool, off=2)
    after = EP._snap_all(h)
    ws, os_ = windows(RR.meta(P["N"], P["rays"], **P["cfg"]), before["state"], ROOTS13, A, dts)
    yield dict(h=h, A=A, dts=dts, pool=pool, full=full, leaf=leaf, scored=scored, first=first, second=second, ws=ws,
               oracles=os_, before=before, after=after)
    close_all(os_)
    pool.close()
    h.close()


def test_stop_state_against_the_oracle(mev, plain):
    P, S = PLAIN, plain
    ws, C = S["ws"], len(ROOTS13)
    assert [w["substeps"] for w in ws] == KS
    cr = crash_at_stop(ws)
    print("crash with a respawn at the stop sub-step: candidates", cr)
    assert cr and any(ws[c]["substeps"] < P["T"] for c in range(C))
    check_slots("scenario 1", S["pool"], np.arange(C), S["oracles"])
    for k in ALL:
        assert G.bits_equal(S["full"][k], S["scored"][k]), k + " differs from mev_evaluate_plans"
    assert G.bits_equal(S["full"]["leaf_obs"], S["leaf"]["leaf_obs"]), "leaf_obs differs from mev_evaluate_leaves"
    for c in range(C):
        EP.check_candidate(f"candidate {c}", S["full"], c, ws[c], P["T"], P["gamma"])
        assert G.bits_equal(S["full"]["leaf_obs"][c], ws[c]["obs"]), f"leaf_obs of candidate {c}"
    # without leaf_obs: the same slots and outputs from the other instantiation
    pool = S["h"].pool(C)
    out = expand(S["h"], S["A"], ROOTS13, S["dts"], P["gamma"], pool, np.arange(C)[::-1].copy(), leaf=False)
    for k in ALL:
        assert G.bits_equal(out[k], S["scored"][k]), k
    check_slots("without leaf_obs", pool, np.arange(C)[::-1].copy(), S["oracles"])
    pool.close()


def test_composition(mev, plain):
    P, S = PLAIN, plain
    C, ws = len(ROOTS13), S["ws"]
    go_on = [c for c in range(C) if ws[c]["substeps"] >= 3]
    assert len(go_on) == 8
    assert sum(ws[c]["substeps"] == P["T"] for c in go_on) == 6 and sum(ws[c]["substeps"] < P["T"] for c in go_on) == 2
    for k in SEQ:  # the first part is the single call's first two rows
        assert G.bits_equal(S["first"][k], S["full"][k][:2]), k
    assert S["first"]["substeps"].tolist() == [min(k, 2) for k in KS]
    check_tail("2 + 3", S["full"], S["second"], go_on, 2)
    same_slots("2 + 3", S["pool"], np.asarray(go_on), np.asarray(go_on) + 2 * C)
    # the candidates that ended in the first part already hold their stop state there
    ended = [c for c in range(C) if c not in go_on]
    same_slots("ended in the first part", S["pool"], np.asarray(ended), np.asarray(ended) + C)


@pytest.mark.parametrize("max_npcs", [32, 64])
def test_traffic_replayed_spawns(mev, max_npcs):
    P = TRAFFIC
    h, ids, roots, A, dts, sp = EP._traffic(mev, max_npcs)
    C, T = P["C"], P["T"]
    state = {k: v.copy() for k, v in h.get_state().items()}
    pool = h.pool(3 * C)
    slots = np.arange(C, dtype=np.int32)
    full = expand(h, A, roots, dts, P["gamma"], pool, slots, sp=sp)
    leaf, scored = EL.both(h, A, roots, dts, P["gamma"], sp)
    ws, os_ = windows(RR.meta(P["N"], P["rays"], **P["cfg"]), state, roots, A, dts, sp, traffic_routes=ids)
    counts = [len(o.get_state()[1]) for o in os_]
    print("NPC counts of the stop states", counts)
    assert max(counts) >= 3 and len(set(counts)) >= 2
    check_slots("traffic", pool, slots, os_)  # (NPC survivors, count and sizes with it)
    for k in ALL:
        assert G.bits_equal(full[k], scored[k]), k
    assert G.bits_equal(full["leaf_obs"], leaf["leaf_obs"])
    # 2 + 2
    first = expand(h, A[:2], roots, dts[:2], P["gamma"], pool, slots + C, sp=sp[:2])
    second = expand(h, A[2:], slots + C, dts[2:], P["gamma"], pool, slots + 2 * C, src=pool, off=2, sp=sp[2:])
    go_on = [c for c in range(C) if ws[c]["substeps"] >= 3]
    assert go_on
    for k in SEQ:
        assert G.bits_equal(first[k], full[k][:2]), k
    check_tail("2 + 2", full, second, go_on, 2)
    same_slots("2 + 2", pool, np.asarray(go_on), np.asarray(go_on) + 2 * C)
    close_all(os_)
    pool.close()
    h.close()


def test_philox_counter_offset(mev):
    """The shape of test_philox_anchor: no spawn_route, so sub-step s draws with the handle's counter +
    counter_offset + (s - 1), keyed by the candidate."""
    E, N, rays, T = 16, 1, 16, 4
    h = EP._handle(mev, E, N, rays, traffic=True, density=20.0, max_steps=0, seed=5)[0]
    rng = np.random.default_rng(6)
    for t in range(12):
        h.step(RR.draw(rng, E, N, 0.5)[0], DT)
    roots = rng.integers(0, E, E).astype(np.int32)
    A, dts, _ = RR.draw_plan(rng, E, N, T, 0.5)
    pool = h.pool(4 * E)
    s = np.arange(E, dtype=np.int32)
    full = expand(h, A, roots, dts, 0.9, pool, s)
    plain_ = h.evaluate_plans(A, roots, dts, 0.9, out=EL.outputs(T, E, N))
    for k in ALL:
        assert G.bits_equal(full[k], plain_[k]), k
    assert (full["substeps"] == T).all()  # (max_steps 0, one ego: nobody ends)
    expand(h, A[:2], roots, dts[:2], 0.9, pool, s + E)
    chained = expand(h, A[2:], s + E, dts[2:], 0.9, pool, s + 2 * E, src=pool, off=2)
    check_tail("offset 2", full, chained, range(E), 2)
    same_slots("offset 2", pool, s, s + 2 * E)
    wrong = expand(h, A[2:], s + E, dts[2:], 0.9, pool, s + 3 * E, src=pool, off=0)
    # the candidates whose second part spawned an NPC, under either counter
    n_mid, n_full, n_wrong = (pool.get_state(q)[0]["npc_count"] for q in (s + E, s, s + 3 * E))
    spawned = np.flatnonzero((n_full > n_mid) | (n_wrong > n_mid))
    print("candidates with a spawn in the second part", spawned.tolist())
    assert spawned.size >= 2
    sf, sw = pool.get_state(spawned)[0], pool.get_state(spawned + 3 * E)[0]
    assert not (G.bits_equal(sf["npc_count"], sw["npc_count"]) and G.bits_equal(sf["npc_x"], sw["npc_x"]) and
                G.bits_equal(wrong["leaf_obs"][spawned], full["leaf_obs"][spawned]))
    pool.close()
    h.close()


def test_twelve_agents_and_car_sizes(mev):
    import torch
    P = TWELVE
    E, N, T, C = P["E"], P["N"], P["T"], P["C"]
    h, _ = EP._handle(mev, E, N, P["rays"], **P["cfg"])
    drng = np.random.default_rng(40)
    sizes = np.stack([drng.uniform(40, 70, (E, N)), drng.uniform(18, 30, (E, N))], -1).astype(np.float32)
    h.set_car_dims(sizes, None)
    EP._device_history_plain(h, P["seed"], steps=12, reset_at={})
    before = EP._snap_all(h)
    rng = np.random.default_rng(P["seed"] + 1)
    roots = [3, 0, 0, 2, 1, 3, 3, 2, 0]
    A, dts, _ = RR.draw_plan(rng, C, N, T, 0.6)
    pool = h.pool(3 * C)
    s = np.arange(C, dtype=np.int32)
    full = expand(h, A, roots, dts, P["gamma"], pool, s)
    ws, os_ = windows(RR.meta(N, P["rays"], **P["cfg"]), before["state"], roots, A, dts, dims=before["dims"])
    check_slots("twelve agents", pool, s, os_)  # (the written sizes are kept in the slots ...
    ed = pool.get_state(s)[1][0]
    assert G.bits_equal(ed, sizes[roots]) and not (ed == np.float32([54.0, 24.0])).all()
    for c in range(C):
        EP.check_candidate(f"candidate {c}", full, c, ws[c], T, P["gamma"])
        assert G.bits_equal(full["leaf_obs"][c], ws[c]["obs"]), f"leaf_obs of candidate {c}"
    expand(h, A[:3], roots, dts[:3], P["gamma"], pool, s + C)
    second = expand(h, A[3:], s + C, dts[3:], P["gamma"], pool, s + 2 * C, src=pool, off=3)
    go_on = [c for c in range(C) if ws[c]["substeps"] > 3]
    assert len(go_on) == C  # (max_steps 2000: nobody ends)
    check_tail("3 + 3", full, second, go_on, 3)  # ... and used from the slots)
    same_slots("3 + 3", pool, s, s + 2 * C)
    EP._assert_same("twelve agents", before, EP._snap_all(h))
    # set_car_dims makes every slot invalid: host mode refuses such a root, device mode makes it a no-op
    h.set_car_dims(sizes, None)
    assert not pool.get_state(np.arange(3 * C))[2].any()
    with pytest.raises(mev._capi.IndexRangeError):
        expand(h, A[3:], s + C, dts[3:], P["gamma"], pool, s + 2 * C, src=pool, off=3)
    torch.cuda.set_device(0)
    dev = "cuda:0"
    o = {k: torch.as_tensor(v).to(dev) for k, v in EL.outputs(3, C, N, h.D).items()}
    h.expand_plans(torch.as_tensor(A[3:]).to(dev).contiguous(), torch.as_tensor(s + C).to(dev), pool,
                   torch.as_tensor(s + 2 * C).to(dev), pool, 3, True, dts[3:], P["gamma"], out=o, device=True)
    h.sync()
    for k in OUT:
        assert not o[k].cpu().numpy().view(np.uint8).any(), k
    assert not pool.get_state(np.arange(3 * C))[2].any()
    close_all(os_)
    pool.close()
    h.close()


def test_capture(mev, plain):
    P, S = PLAIN, plain
    h, C = S["h"], len(ROOTS13)
    pool = h.pool(P["E"] + C + 2)
    envs = np.asarray([5, 0, 3, 1, 4, 2], np.int32)
    at = np.asarray([0, 2, 1, 5, 3, 4], np.int32)  # env envs[i] -> slot at[i]
    pool.capture(envs, at)
    st, dims, valid = pool.get_state(at)
    assert valid.all() and not pool.get_state([P["E"], P["E"] + C + 1])[2].any()
    live = S["before"]["state"]
    for name in st:
        assert G.bits_equal(st[name], live[name][envs]), name
    assert G.bits_equal(dims[0], S["before"]["dims"][0][envs])
    # expanding the captured slots equals expanding the live envs; src == dst, children in fresh slots
    slot_of = {int(e): int(q) for e, q in zip(envs, at)}
    roots = np.asarray([slot_of[r] for r in ROOTS13], np.int32)
    kids = np.arange(C, dtype=np.int32) + P["E"]
    out = expand(h, S["A"], roots, S["dts"], P["gamma"], pool, kids, src=pool)
    for k in OUT:
        assert G.bits_equal(out[k], S["full"][k]), k
    check_slots("from captured slots", pool, kids, S["oracles"])
    # device pointers, and pairs out of range skipped
    import torch
    torch.cuda.set_device(0)
    fresh = h.pool(4)
    e_d = torch.as_tensor(np.asarray([1, P["E"], 2, -1], np.int32)).to("cuda:0")
    s_d = torch.as_tensor(np.asarray([3, 0, 4, 1], np.int32)).to("cuda:0")
    fresh.capture(e_d, s_d, device=True)
    h.sync()
    st, _, valid = fresh.get_state(np.arange(4))
    assert valid.tolist() == [0, 0, 0, 1] and G.bits_equal(st["x"][3], live["x"][1])
    with pytest.raises(mev._capi.IndexRangeError):
        fresh.capture([0, 1], [0, 4])
    with pytest.raises(mev._capi.IndexRangeError):
        fresh.capture([0, P["E"]], [0, 1])
    assert fresh.get_state(np.arange(4))[2].tolist() == [0, 0, 0, 1]
    fresh.close()
    pool.close()
    EP._assert_same("capture", S["before"], EP._snap_all(h))


def test_handle_untouched_no_traffic(mev, plain):
    P, S = PLAIN, plain
    EP._assert_same("scenario 1", S["before"], S["after"])

    def twin():
        t, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
        EP._device_history_plain(t, P["seed"])
        return t

    h = twin()  # (on a copy: the shared scenario's handle stays where the other tests expect it)
    pool = h.pool(13)
    out = expand(h, S["A"], ROOTS13, S["dts"], P["gamma"], pool, np.arange(13))
    for k in OUT:
        assert G.bits_equal(out[k], S["full"][k]), k
    EP._twin_step("scenario 1", mev, h, twin, P["N"])
    pool.close()
    h.close()


def test_handle_untouched_traffic(mev):
    P = TRAFFIC
    h, ids, roots, A, dts, sp = EP._traffic(mev, 32)
    C = P["C"]
    before = EP._snap_all(h)
    pool = h.pool(2 * C)
    s = np.arange(C, dtype=np.int32)
    expand(h, A, roots, dts, P["gamma"], pool, s, sp=sp)
    expand(h, A, roots, dts, P["gamma"], pool, s, leaf=False)  # (and with the Philox spawner)
    expand(h, A, s, dts, P["gamma"], pool, s + C, src=pool, off=4)
    EP._assert_same("traffic", before, EP._snap_all(h))

    def twin():
        t, _ = EP._handle(mev, P["E"], P["N"], P["rays"], max_npcs=32, **P["cfg"])
        EP._device_history_traffic(t, P["seed"])
        return t

    EP._twin_step("traffic", mev, h, twin, P["N"])
    pool.close()
    h.close()


def test_device_pointers(mev, plain):
    """The second level of scenario 1 with device pointers, into fresh slots of another pool."""
    import torch
    torch.cuda.set_device(0)
    P, S = PLAIN, plain
    h, C, N, T2, dev = S["h"], len(ROOTS13), P["N"], 3, "cuda:0"
    src = S["pool"]
    tA = torch.as_tensor(S["A"][2:]).to(dev).contiguous()
    dts = S["dts"][2:]

    def call(roots, dst_slots, dst):
        o = {k: torch.as_tensor(v).to(dev) for k, v in EL.outputs(T2, C, N, h.D).items()}
        h.expand_plans(tA, torch.as_tensor(np.asarray(roots, np.int32)).to(dev), dst,
                       torch.as_tensor(np.asarray(dst_slots, np.int32)).to(dev), src, 2, True, dts, P["gamma"], out=o,
                       device=True)
        h.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    roots = np.arange(C) + C
    a = h.pool(C)
    got = call(roots, np.arange(C), a)
    for k in OUT:
        assert G.bits_equal(got[k], S["second"][k]), k
    same = [c for c in range(C)]
    (sa, da, va), (sb, db, vb) = a.get_state(same), src.get_state(np.arange(C) + 2 * C)
    assert va.all() and vb.all() and G.bits_equal(da[0], db[0])
    for name in sa:
        assert G.bits_equal(sa[name], sb[name]), name  # (no traffic: the NPC slots are the root's, zero)
    # a root out of range, a root slot nothing was stored in, a stop state not kept
    b = h.pool(C)
    bad_roots, bad_dst = roots.copy(), np.arange(C)
    bad_roots[4], bad_roots[9], bad_dst[2] = src.slots, 47, -1
    got = call(bad_roots, bad_dst, b)
    for k in OUT:
        want = S["second"][k].copy()
        if k in SEQ:
            want[:, [4, 9]] = 0
        else:
            want[[4, 9]] = 0
        assert G.bits_equal(got[k], want), k
    valid = b.get_state(np.arange(C))[2]
    assert valid.tolist() == [0 if c in (2, 4, 9) else 1 for c in range(C)]
    keep = [c for c in range(C) if c not in (2, 4, 9)]
    sa, sb = a.get_state(keep)[0], b.get_state(keep)[0]
    for name in sa:
        assert G.bits_equal(sa[name], sb[name]), name
    assert not any(x.view(np.uint8).any() for x in b.get_state([2, 4, 9])[0].values())  # (as created: zero)
    # only the pool as an output
    c_ = h.pool(C)
    h.expand_plans(tA, torch.as_tensor(roots.astype(np.int32)).to(dev), c_, torch.as_tensor(np.arange(C, dtype=np.int32)).to(dev),
                   src, 2, False, dts, P["gamma"], out={}, device=True)
    h.sync()
    sc = c_.get_state(same)[0]
    for name in sa:
        assert G.bits_equal(sc[name], a.get_state(same)[0][name]), name
    for q in (a, b, c_):
        q.close()
    EP._assert_same("device calls", S["before"], EP._snap_all(h))


def test_chunks(mev, plain, monkeypatch):
    """MEV_LEAF_CHUNK=4 at creation: 13 candidates in chunks of 4, 4, 4 and 1, outputs and slots the same."""
    P, S = PLAIN, plain
    monkeypatch.setenv("MEV_LEAF_CHUNK", "4")
    h, _ = EP._handle(mev, P["E"], P["N"], P["rays"], **P["cfg"])
    monkeypatch.delenv("MEV_LEAF_CHUNK")
    EP._device_history_plain(h, P["seed"])
    pool = h.pool(13)
    out = expand(h, S["A"], ROOTS13, S["dts"], P["gamma"], pool, np.arange(13))
    for k in OUT:
        assert G.bits_equal(out[k], S["full"][k]), k
    check_slots("chunks", pool, np.arange(13), S["oracles"])
    pool.close()
    h.close()


def test_errors(mev):
    E, N, rays, T, C = 2, 1, 16, 3, 2
    cfg = dict(use_team=False, max_steps=0)
    h, _ = EP._handle(mev, E, N, rays, **cfg)
    other, _ = EP._handle(mev, E, N, rays, **cfg)
    EP._device_history_plain(h, 35, steps=5, reset_at={})
    pool, foreign = h.pool(6), other.pool(6)
    pool.capture([0, 1], [0, 1])
    A, dts, _ = RR.draw_plan(np.random.default_rng(36), C, N, T, 0.6)
    before = EP._snap_all(h)
    slots = np.arange(6)
    pb = pool.get_state(slots)

    def call(roots=(0, 1), dst=pool, dst_slots=(2, 3), src=None, **kw):
        return h.expand_plans(A, roots, dst, dst_slots, src, dt=dts, **kw)

    for bad in (dict(dst_slots=(2, 2)),                    # a slot twice
                dict(src=pool, dst_slots=(1, 2)),          # a dst slot that is a root, in one pool
                dict(dst=foreign), dict(src=foreign),      # a pool of another handle
                dict(dst=None),                            # a null dst
                dict(flags=mev._capi.MEV_AUTO_RESET)):
        with pytest.raises(mev.MevError) as ei:
            call(**bad)
        assert not isinstance(ei.value, mev._capi.IndexRangeError), bad
    for bad in (dict(dst_slots=(2, 6)), dict(dst_slots=(-2, 3)),  # slots outside the range
                dict(roots=(0, E)), dict(src=pool, roots=(0, 6)), dict(src=pool, roots=(0, -1)),
                dict(src=pool, roots=(0, 4))):                    # a slot nothing was stored in
        with pytest.raises(mev._capi.IndexRangeError):
            call(**bad)
    with pytest.raises(ValueError):
        call(dst_slots=(2, 3, 4))
    with pytest.raises(mev.MevError):
        h.pool(0)
    EP._assert_same("refused calls", before, EP._snap_all(h))
    pa = pool.get_state(slots)
    for name in pb[0]:
        assert G.bits_equal(pb[0][name], pa[0][name]), name
    assert pa[2].tolist() == [1, 1, 0, 0, 0, 0] and G.bits_equal(pb[1][0], pa[1][0])
    # -1 keeps nothing; a valid call works after the refused ones, with src == dst
    out = call(src=pool, dst_slots=(-1, 5))
    assert pool.get_state(slots)[2].tolist() == [1, 1, 0, 0, 0, 1] and (out["substeps"] == T).all()
    foreign.close()
    other.close()
    pool.close()
    pool.close()  # (twice: a no-op)
    late = h.pool(2)
    h.close()     # (releases `late` too)
    late.close()


def test_interplay_with_the_step_server(mev):
    E, N, rays, T, C = 2, 2, 16, 3, 5
    cfg = dict(use_team=True, max_steps=40)
    meta = RR.meta(N, rays, **cfg)
    h = RR.handle(mev, E, N, rays, **cfg)
    ref = RR.start(h, meta)
    rng = np.random.default_rng(8)

    def plain_step(tag):
        a, _ = RR.draw(rng, E, N, 0.6)
        out = h.step(a, DT, auto_reset=True)
        ws = ref.step(a[None], [DT])
        for e in range(E):
            R.check_step(f"{tag} env {e}", out, e, ws[e])

    plain_step("served step")
    assert h.serve_stats()["steps"] == 1 and h.serve_stats()["running"]
    pool = h.pool(C)
    assert h.serve_stats()["running"] == 0
    plain_step("served again")
    assert h.serve_stats()["running"]
    A, dts, _ = RR.draw_plan(rng, C, N, T, 0.6)
    roots = [1, 0, 0, 1, 1]
    out = expand(h, A, roots, dts, 0.9, pool, np.arange(C))
    assert h.serve_stats()["running"] == 0
    ws, os_ = windows(meta, h.get_state(), roots, A, dts)
    for c in range(C):
        EP.check_candidate(f"after a served step, candidate {c}", out, c, ws[c], T, 0.9)
    check_slots("after a served step", pool, np.arange(C), os_)
    plain_step("step after the call")
    close_all(os_)
    pool.close()
    h.close()
    ref.close()


def _two_level_tree(mev, backend):
    """A two-level tree: C1 first plans per env into slots, C2 continuations per slot; the best leaf's
    return sequence equals a step_sequence of the concatenated winning plan on a twin."""
    import pkgload
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, rays, T, B1, B2 = 2, 2, 16, 2, 3, 2
    kw = dict(lidar_rays=rays, use_team_reward=True, max_steps=50, backend=backend)
    v, twin = (vec_env.VecIntersectionEnv(E, N, **kw) for _ in range(2))
    rng = np.random.default_rng(11)
    for x in (v, twin):
        RR.set_routes(x.handle)
    for t in range(3):
        a = RR.draw(rng, E, N, 0.6)[0]
        v.step(a)
        twin.step(a)
    C1, C2 = E * B1, E * B1 * B2
    pool = v.make_pool(C1 + C2)
    roots1 = np.repeat(np.arange(E), B1).astype(np.int32)
    A1, dts1, _ = RR.draw_plan(rng, C1, N, T, 0.6)
    l1 = v.expand_plans(A1, roots1, pool, np.arange(C1, dtype=np.int32), dt=dts1, gamma=0.9, copy=True)
    roots2 = np.repeat(np.arange(C1), B2).astype(np.int32)
    A2, dts2, _ = RR.draw_plan(rng, C2, N, T, 0.6)
    l2 = v.expand_plans(A2, roots2, pool, C1 + np.arange(C2, dtype=np.int32), src=pool, counter_offset=T, dt=dts2,
                        gamma=0.9, leaf_obs=True, copy=True)
    assert set(l2) == set(OUT)
    if backend == "torch":
        l1, l2 = ({k: x.cpu().numpy() for k, x in d.items()} for d in (l1, l2))
    assert (l1["substeps"] == T).all() and (l2["substeps"] == T).all()
    # per env the leaf with the best team return over both levels (g restarts at 1 in the second call)
    g2 = np.float32(0.9) ** T
    total = l1["returns"].sum(1)[roots2] + g2 * l2["returns"].sum(1)
    plan = np.zeros((2 * T, E, N, 2), np.float32)
    best = []
    for e in range(E):
        mine = np.flatnonzero(roots1[roots2] == e)
        b = int(mine[np.argmax(total[mine])])
        best.append(b)
        plan[:T, e], plan[T:, e] = A1[:, roots2[b]], A2[:, b]
    obs, rew, term, trunc, info = twin.step_sequence(plan, dt=np.concatenate([dts1, dts2]))
    rs = info["reward_seq"].cpu().numpy() if backend == "torch" else info["reward_seq"]
    obs = obs.cpu().numpy() if backend == "torch" else obs
    for e, b in enumerate(best):
        assert G.bits_equal(rs[:T, e], l1["reward_seq"][:, roots2[b]]), f"env {e}: first level rows"
        assert G.bits_equal(rs[T:, e], l2["reward_seq"][:, b]), f"env {e}: second level rows"
        assert G.bits_equal(obs[e], l2["leaf_obs"][b]), f"env {e}: leaf observation"
    st, _, valid = pool.get_state(C1 + np.asarray(best))
    tw = twin.handle.get_state()
    assert valid.all()
    for name in ("x", "y", "v", "heading", "path_index", "prev_dist", "step_count"):
        assert G.bits_equal(st[name], tw[name]), name
    pool.close()
    v.close()
    twin.close()


def test_vec_env_numpy_two_level_tree(mev):
    _two_level_tree(mev, "numpy")


def test_vec_env_torch_two_level_tree(mev):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the device")
    _two_level_tree(mev, "torch")
