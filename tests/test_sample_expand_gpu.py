"""mev_sample_expand_plans (include/marlenv.h): mev_sample_plans whose groups may start from slots of a
pool and whose candidates' stop states are kept in one.  Its contract is two equalities, both checked
bit for bit: actions_out against the numpy restatement of the stated formula (plan_noise_ref), and
every other output, leaf_obs and every stored slot against mev_expand_plans on the same handle fed
actions_out, the groups' roots repeated per candidate and the same src, dst_slots and counter_offset
-- a call whose own tests check it against the oracle; the slots are checked against the oracle here
as well.  Every output buffer is filled with 0xFF bytes before a call.

The shared scene is test_sample_plans_gpu's (6 envs, 16 beams, T = 5, K = 5, roots [0, 3, 3, 5],
max_steps = 20: the candidates of env 0 stop at their first sub-step, those of env 3 are truncated at
the third, those of env 5 run all rows); helpers are those of test_evaluate_plans_gpu,
test_expand_plans_gpu and test_sample_plans_gpu, imported.

Chosen on the CPU with the oracle alone (the history replayed by oracles, the actions from
plan_noise_ref): from the shared scene's roots no action within the clamp makes any car crash inside
five sub-steps, for N = 2 and N = 12 alike, so the composition test runs the same scene after the
history drawn with seed 21 (N = 12).  There, level 1 (the first two rows of the shared distribution)
followed by level 2 (distribution seed 60, noise counter COUNTER + 7) gives the sub-step counts
[1] * 5 + [3] * 10 + [5] * 5, and candidate 12 -- which goes on into level 2 and is truncated at its
third sub-step -- crashes and respawns in that sub-step."""
import ctypes

import numpy as np
import pytest

import golden_replay as G
import plan_noise_ref as PN
import test_evaluate_leaves_gpu as EL
import test_evaluate_plans_gpu as EP
import test_expand_plans_gpu as XP
import test_sample_plans_gpu as SP
import window_ref as RR
from test_sample_plans_gpu import C, COUNTER, DTS, E, GAMMA, GROUPS, HI, K, LO, RAYS, ROOTS, SEED, T
from window_ref import DT

pytestmark = pytest.mark.gpu

ALL, SEQ = EP.ALL, EP.SEQ
OUT = ALL + ("leaf_obs",)
SLOTS = np.arange(C, dtype=np.int32)
HISTORY2, DIST2, COUNTER2, T1 = 21, 60, COUNTER + 7, 2  # the composition test (chosen on the CPU, see above)


# ---- helpers ----

def buffers(Tn, Cn, N, D=None):
    """Every output of the call, 0xFF bytes."""
    return dict(EL.outputs(Tn, Cn, N, D), actions_out=EL.filled((Tn, Cn, N, 2), np.float32))


def sample_expand(h, mean, sigma, dst, dst_slots, roots=ROOTS, samples=K, src=None, off=0, leaf=True, **kw):
    Tn, Cn = mean.shape[0], mean.shape[1] * samples
    args = dict(dt=DTS[:Tn], gamma=GAMMA, lo=LO, hi=HI, seed=SEED, counter=COUNTER, leaf_obs=leaf,
                out=buffers(Tn, Cn, h.N, h.D if leaf else None), src=src, dst=dst, dst_slots=dst_slots, counter_offset=off)
    args.update(kw)
    return h.sample_plans(mean, sigma, roots, samples, **args)


class _Two:
    """Two pools behind XP.same_slots' one: its first read-back goes to the first, its second to the other."""

    def __init__(self, first, second):
        self.pools = [first, second]

    def get_state(self, slots):
        return self.pools.pop(0).get_state(slots)


def same_slots(tag, pa, a, pb, b):
    XP.same_slots(tag, _Two(pa, pb), np.asarray(a), np.asarray(b))


def assert_equals_expand(tag, h, out, roots, pool, slots, ref_pool, samples=K, dts=DTS, src=None, off=0, leaf=True, sp=None,
                         stored=None):
    """`out` and the slots it left in `pool` against mev_expand_plans fed out's actions into ref_pool."""
    A = out["actions_out"]
    ref = XP.expand(h, A, np.repeat(roots, samples).astype(np.int32), dts[:A.shape[0]], GAMMA, ref_pool, slots, src, off, sp, leaf)
    for k in ALL + (("leaf_obs",) if leaf else ()):
        assert G.bits_equal(out[k], ref[k]), f"{tag}: {k}"
    keep = np.asarray(slots)[np.asarray(slots) >= 0] if stored is None else stored
    same_slots(tag, pool, keep, ref_pool, keep)
    return ref


def formula(mean, sigma, samples=K, counter=COUNTER, **kw):
    return PN.sampled_actions(mean, sigma, samples, LO, HI, SEED, counter, **kw)


# ---- the shared scene (computed once, never changed): pool `a` holds the call's 20 stop states from
# the live batch, pool `b` those of mev_expand_plans on its actions ----

@pytest.fixture(scope="module", params=[2, 12])
def scene(mev, request):
    N = request.param
    h = SP.make_handle(mev, N)
    before = EP._snap_all(h)
    mean, sigma = SP.draw_dist(N)
    a, b = h.pool(C), h.pool(C)
    out = sample_expand(h, mean, sigma, a, SLOTS)
    after = EP._snap_all(h)
    yield dict(h=h, N=N, mean=mean, sigma=sigma, out=out, a=a, b=b, before=before, after=after)
    h.close()


# 1
def test_from_the_live_batch(scene):
    S = scene
    h, N, out = S["h"], S["N"], S["out"]
    assert list(S["before"]["state"]["step_count"][ROOTS]) == [25, 17, 17, 10]
    assert out["actions_out"].shape == (T, C, N, 2)
    assert G.bits_equal(out["actions_out"], formula(S["mean"], S["sigma"]))  # (every row: also after an early stop)
    assert out["substeps"].tolist() == [1] * K + [3] * (2 * K) + [T] * K
    assert_equals_expand("with leaf_obs", h, out, ROOTS, S["a"], SLOTS, S["b"])
    # the sampled call itself, which keeps nothing, returns the same
    plain = SP.sample(h, S["mean"], S["sigma"])
    for k in OUT + ("actions_out",):
        assert G.bits_equal(out[k], plain[k]), k
    # without leaf_obs: the other instantiation, the same outputs and slots
    c = h.pool(C)
    bare = sample_expand(h, S["mean"], S["sigma"], c, SLOTS[::-1].copy(), leaf=False)
    assert "leaf_obs" not in bare
    for k in ALL + ("actions_out",):
        assert G.bits_equal(bare[k], out[k]), k
    same_slots("without leaf_obs", c, SLOTS[::-1], S["b"], SLOTS)
    c.close()
    # each slot against the oracle that ran the candidate's window from its root's state
    roots = np.repeat(ROOTS, K)
    ws, os_ = XP.windows(RR.meta(N, RAYS, **SP.CFG), S["before"]["state"], roots, out["actions_out"], DTS)
    XP.check_slots("live batch", S["a"], SLOTS, os_)
    for c_ in range(C):
        EP.check_candidate(f"candidate {c_}", out, c_, ws[c_], T, GAMMA)
        assert G.bits_equal(out["leaf_obs"][c_], ws[c_]["obs"]), f"leaf_obs of candidate {c_}"
    XP.close_all(os_)
    EP._assert_same("scene", S["before"], EP._snap_all(h))


# 2
def test_from_a_pool_and_composition(mev):
    N, T2 = 12, T - T1
    h, _ = EP._handle(mev, E, N, RAYS, **SP.CFG)
    EP._device_history_plain(h, HISTORY2)
    before = EP._snap_all(h)
    assert list(before["state"]["step_count"][ROOTS]) == [25, 17, 17, 10]
    top, tree, ref_pool = h.pool(GROUPS), h.pool(2 * C), h.pool(C)
    top.capture(ROOTS, np.arange(GROUPS))
    mean, sigma = SP.draw_dist(N)
    l1 = sample_expand(h, mean[:T1], sigma[:T1], tree, SLOTS, roots=np.arange(GROUPS, dtype=np.int32), src=top)
    assert G.bits_equal(l1["actions_out"], formula(mean[:T1], sigma[:T1]))
    m2, s2 = SP.draw_dist(N, seed=DIST2, groups=C, t=T2)
    l2 = sample_expand(h, m2, s2, tree, SLOTS + C, roots=SLOTS, samples=1, src=tree, off=T1, counter=COUNTER2, dt=DTS[T1:])
    assert G.bits_equal(l2["actions_out"], formula(m2, s2, samples=1, counter=COUNTER2))
    # the single call from the live roots with the two levels' actions, and the oracle's windows
    A = np.concatenate([l1["actions_out"], l2["actions_out"]])
    roots = np.repeat(ROOTS, K).astype(np.int32)
    full = XP.expand(h, A, roots, DTS, GAMMA, ref_pool, SLOTS)
    scored = h.evaluate_plans(A, roots, DTS, GAMMA, out=EL.outputs(T, C, N, h.D), leaf_obs=True)
    for k in OUT:
        assert G.bits_equal(full[k], scored[k]), k
    ws, os_ = XP.windows(RR.meta(N, RAYS, **SP.CFG), before["state"], roots, A, DTS)
    ks = [w["substeps"] for w in ws]
    assert ks == [1] * K + [3] * (2 * K) + [T] * K
    go_on = [c for c in range(C) if ks[c] > T1]
    ended = [c for c in range(C) if ks[c] <= T1]
    crashed = XP.crash_at_stop(ws)
    print("go on", go_on, "ended in level 1", ended, "crash with a respawn at the stop sub-step", crashed)
    assert go_on and ended and set(crashed) & set(go_on)
    # level 1 is the single call's first rows; level 2 its tail, for the candidates that went on
    for k in SEQ:
        assert G.bits_equal(l1[k], full[k][:T1]), k
    assert l1["substeps"].tolist() == [min(k, T1) for k in ks]
    XP.check_tail("2 + 3", full, l2, go_on, T1)
    same_slots("2 + 3", tree, np.asarray(go_on) + C, ref_pool, go_on)
    XP.check_slots("2 + 3 against the oracle", tree, np.asarray(go_on) + C, [os_[c] for c in go_on])
    # the candidates that ended in level 1 hold their stop state there
    same_slots("ended in level 1", tree, ended, ref_pool, ended)
    # each level equals mev_expand_plans on its own actions
    p1, p2 = h.pool(C), h.pool(C)
    assert_equals_expand("level 1", h, l1, np.arange(GROUPS), tree, SLOTS, p1, src=top)
    x2 = XP.expand(h, l2["actions_out"], SLOTS, DTS[T1:], GAMMA, p2, SLOTS, tree, T1)
    for k in OUT:
        assert G.bits_equal(l2[k], x2[k]), k
    same_slots("level 2", tree, SLOTS + C, p2, SLOTS)
    EP._assert_same("composition", before, EP._snap_all(h))
    XP.close_all(os_)
    h.close()


# 3
def test_one_pool_as_source_and_destination(scene):
    S = scene
    h = S["h"]
    one = h.pool(GROUPS + C)
    one.capture(ROOTS, np.arange(GROUPS))
    out = sample_expand(h, S["mean"], S["sigma"], one, SLOTS + GROUPS, roots=np.arange(GROUPS, dtype=np.int32), src=one)
    for k in OUT + ("actions_out",):
        assert G.bits_equal(out[k], S["out"][k]), k
    same_slots("src == dst", one, SLOTS + GROUPS, S["a"], SLOTS)
    assert one.get_state(np.arange(GROUPS))[2].all()
    one.close()


# 4
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("max_npcs", [32, 64])
def test_traffic(mev, max_npcs, N):
    """Dense traffic: the Philox spawner at a counter offset, a replayed spawn_route, and no leaf_obs."""
    En, Tn, Gn = 8, 4, 5
    Cn = Gn * K
    h, _ = EP._handle(mev, En, N, RAYS, max_npcs=max_npcs, traffic=True, density=20.0, max_steps=2000)
    EP._device_history_traffic(h, EP.TRAFFIC["seed"])
    before = EP._snap_all(h)
    assert before["state"]["npc_count"].max() >= 3
    rng = np.random.default_rng(51)
    roots = rng.integers(0, En, Gn).astype(np.int32)
    mean, sigma = SP.draw_dist(N, seed=52, groups=Gn, t=Tn)
    sp = rng.integers(-1, 12, (Tn, Cn))
    slots = np.arange(Cn, dtype=np.int32)
    pool, ref = h.pool(Cn), h.pool(Cn)
    counts = []
    for tag, kw in (("philox spawner, offset 3", dict(off=3)), ("spawn_route", dict(sp=sp)),
                    ("no leaf_obs", dict(off=1, leaf=False))):
        out = sample_expand(h, mean, sigma, pool, slots, roots=roots, off=kw.get("off", 0), leaf=kw.get("leaf", True),
                            spawn_route=kw.get("sp"))
        assert G.bits_equal(out["actions_out"], formula(mean, sigma)), tag
        assert_equals_expand(tag, h, out, roots, pool, slots, ref, **kw)  # (NPC survivors, counts and sizes with it)
        counts.append(pool.get_state(slots)[0]["npc_count"].copy())
    print("NPC counts of the stop states", [c.tolist() for c in counts])
    assert all(c.max() >= 1 for c in counts)  # (survivors in the slots that were compared)
    EP._assert_same("traffic", before, EP._snap_all(h))
    h.close()


# 5
def test_car_sizes(mev):
    N = 3
    h = SP.make_handle(mev, N, dims=True)
    assert h.car_dims_active()
    sizes = h.car_dims()[0]
    mean, sigma = SP.draw_dist(N)
    pool, ref = h.pool(C), h.pool(C)
    out = sample_expand(h, mean, sigma, pool, SLOTS)
    assert G.bits_equal(out["actions_out"], formula(mean, sigma))
    assert_equals_expand("per-car sizes", h, out, ROOTS, pool, SLOTS, ref)
    kept = pool.get_state(SLOTS)[1][0]
    assert G.bits_equal(kept, sizes[np.repeat(ROOTS, K)]) and not (kept == np.float32([54.0, 24.0])).all()
    h.close()


# 6
def test_chunks_cut_through_groups(mev, scene, monkeypatch):
    """MEV_LEAF_CHUNK=3 at creation, K = 5: 20 candidates in chunks of 3, outputs and slots the same."""
    S = scene
    monkeypatch.setenv("MEV_LEAF_CHUNK", "3")
    h = SP.make_handle(mev, S["N"])
    monkeypatch.delenv("MEV_LEAF_CHUNK")
    pool = h.pool(C)
    out = sample_expand(h, S["mean"], S["sigma"], pool, SLOTS)
    for k in OUT + ("actions_out",):
        assert G.bits_equal(out[k], S["out"][k]), k
    same_slots("chunks", pool, SLOTS, S["a"], SLOTS)
    h.close()


# 7
def test_mean_first_and_slots_not_stored(scene):
    S = scene
    h, mean, sigma, base = S["h"], S["mean"], S["sigma"], S["out"]
    pool, ref = h.pool(C), h.pool(C)
    out = sample_expand(h, mean, sigma, pool, SLOTS, mean_first=True)
    a = out["actions_out"]
    clamped = np.minimum(np.maximum(mean + np.float32(0.0) * sigma, np.float32(LO)), np.float32(HI)).astype(np.float32)
    assert G.bits_equal(a[:, ::K], clamped)
    assert G.bits_equal(a, formula(mean, sigma, mean_first=True))
    others = np.arange(C) % K != 0
    assert G.bits_equal(a[:, others], base["actions_out"][:, others])
    assert_equals_expand("mean first", h, out, ROOTS, pool, SLOTS, ref)
    same_slots("mean first, the other candidates", pool, SLOTS[others], S["a"], SLOTS[others])
    # dst_slots = -1: slot 7 keeps the env captured into it, slots 1 and 13 stay as created
    part = h.pool(C)
    part.capture([1], [7])
    skip = [1, 7, 13]
    was = part.get_state(skip)
    slots = SLOTS.copy()
    slots[skip] = -1
    out = sample_expand(h, mean, sigma, part, slots)
    for k in OUT + ("actions_out",):
        assert G.bits_equal(out[k], base[k]), k
    now = part.get_state(skip)
    assert now[2].tolist() == [0, 1, 0]
    for name in was[0]:
        assert G.bits_equal(was[0][name], now[0][name]), name
    assert G.bits_equal(was[1][0], now[1][0]) and G.bits_equal(was[1][1], now[1][1])
    assert not any(x[[0, 2]].view(np.uint8).any() for x in now[0].values())  # (as created: zero)
    stored = slots[slots >= 0]
    assert part.get_state(stored)[2].all()
    same_slots("the slots that were stored", part, stored, S["a"], stored)
    for q in (pool, ref, part):
        q.close()


# 8
def test_device_pointers(mev, scene):
    import torch
    torch.cuda.set_device(0)
    S = scene
    N, base, dev = S["N"], S["out"], "cuda:0"
    h = SP.make_handle(mev, N)  # (a copy: this test moves the handle to a stream of its own)
    stream = torch.cuda.Stream(device=0)
    h.set_stream(stream.cuda_stream)
    keys = OUT + ("actions_out",)

    def call(roots, dst, dst_slots, src=None, out=None, wait=False, leaf=True):
        o = {k: torch.as_tensor(v).to(dev) for k, v in buffers(T, C, N, h.D).items()} if out is None else out
        args = [torch.as_tensor(x).to(dev) for x in (S["mean"], S["sigma"], np.asarray(roots, np.int32),
                                                     np.asarray(dst_slots, np.int32))]
        torch.cuda.synchronize()
        if wait:  # work ahead of the call on its stream: a call that synchronised would return after it
            with torch.cuda.stream(stream):
                torch.cuda._sleep(5_000_000)
        SP.sample(h, args[0], args[1], roots=args[2], out=o, device=True, leaf=leaf, src=src, dst=dst, dst_slots=args[3])
        pending = not stream.query()
        h.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}, pending

    # the host-mode results, and no synchronisation
    a = h.pool(C)
    got, pending = call(ROOTS, a, SLOTS, wait=True)
    assert pending, "the call returned only after the work queued ahead of it"
    for k in keys:
        assert G.bits_equal(got[k], base[k]), k
    same_slots("device pointers", a, SLOTS, S["a"], SLOTS)
    # from a pool: group 1 rooted at a slot nothing was stored in, group 3 out of range -- all-zero
    # outputs for their K candidates, the formula's action rows, nothing stored; dst_slots out of
    # range store nothing either
    top, b = h.pool(GROUPS + 2), h.pool(C)
    top.capture(ROOTS, np.arange(GROUPS))
    roots = np.array([0, GROUPS, 2, GROUPS + 2], np.int32)
    slots = SLOTS.copy()
    slots[[11, 12]] = C, -5
    got, _ = call(roots, b, slots, src=top)
    gone = np.r_[K:2 * K, 3 * K:4 * K]
    for k in keys:
        want = base[k].copy()
        if k in SEQ:
            want[:, gone] = 0
        elif k != "actions_out":
            want[gone] = 0
        assert G.bits_equal(got[k], want), k
    empty = sorted(gone.tolist() + [11, 12])
    assert b.get_state(SLOTS)[2].tolist() == [0 if c in empty else 1 for c in range(C)]
    assert not any(x.view(np.uint8).any() for x in b.get_state(empty)[0].values())  # (as created: zero)
    kept = [c for c in range(C) if c not in empty]
    same_slots("beside the groups without a root", b, kept, S["a"], kept)
    # only the pool as an output
    c_ = h.pool(C)
    call(ROOTS, c_, SLOTS, out={}, leaf=False)
    same_slots("only the pool", c_, SLOTS, S["a"], SLOTS)
    h.close()


# 9
def test_handle_untouched(mev, scene):
    S = scene
    EP._assert_same("sample_expand", S["before"], S["after"])
    if S["N"] != 2:
        return
    h = SP.make_handle(mev, 2)  # (a copy: the shared scene's handle stays where the other tests expect it)
    pool = h.pool(C)
    out = sample_expand(h, S["mean"], S["sigma"], pool, SLOTS)
    for k in OUT + ("actions_out",):
        assert G.bits_equal(out[k], S["out"][k]), k
    EP._twin_step("sample_expand", mev, h, lambda: SP.make_handle(mev, 2), 2)
    h.close()


# 10
def test_errors(mev):
    N, Gn, Kn, Tn = 1, 2, 2, 3
    cfg = dict(use_team=False, max_steps=0)
    h, _ = EP._handle(mev, 2, N, RAYS, **cfg)
    other, _ = EP._handle(mev, 2, N, RAYS, **cfg)
    EP._device_history_plain(h, 35, steps=5, reset_at={})
    pool, foreign = h.pool(8), other.pool(8)
    pool.capture([0, 1], [0, 1])
    mean, sigma = SP.draw_dist(N, groups=Gn, t=Tn)
    before = EP._snap_all(h)
    every = np.arange(8)
    pb = pool.get_state(every)
    lib, cap = mev.load_library(), mev._capi

    def call(roots=(0, 1), dst=pool, dst_slots=(2, 3, 4, 5), src=None, **kw):
        args = dict(dt=DT, lo=LO, hi=HI, seed=1, counter=2, src=src, dst=dst, dst_slots=dst_slots)
        return h.sample_plans(mean, sigma, roots, Kn, **dict(args, **kw))

    def refused(code, words, **bad):
        with pytest.raises(mev.MevError) as ei:
            call(**bad)
        assert isinstance(ei.value, cap.IndexRangeError) == (code == -4), bad
        assert any(w in str(ei.value) for w in words), (bad, str(ei.value))

    refused(-1, ["dst_slots required"], dst_slots=None)                        # a null dst_slots
    refused(-1, ["another handle"], dst=foreign)                               # a foreign pool
    refused(-1, ["another handle"], src=foreign)
    refused(-1, ["twice"], dst_slots=(2, 3, 3, 5))                             # a slot named twice
    refused(-1, ["is a root"], src=pool, dst_slots=(2, 1, 4, 5))               # a dst slot that is a root, in one pool
    refused(-4, ["dst_slots[3]"], dst_slots=(2, 3, 4, 8))                      # dst_slots out of range
    refused(-4, ["dst_slots[0]"], dst_slots=(-2, 3, 4, 5))
    refused(-4, ["roots[1]"], roots=(0, 2))                                    # a root outside the live batch
    refused(-4, ["roots[1]"], src=pool, roots=(0, 8))                          # ... outside the source pool
    refused(-4, ["roots[0]"], src=pool, roots=(-1, 0))
    refused(-4, ["nothing valid"], src=pool, roots=(0, 6))                     # an invalid source slot
    refused(-1, ["MEV_DEVICE_PTRS only"], flags=cap.MEV_AUTO_RESET)
    refused(-1, ["lo and hi"], lo=(0.8, -1.0))
    with pytest.raises(ValueError):
        call(dst_slots=(2, 3, 4))
    with pytest.raises(ValueError):
        call(dst=None)           # (dst_slots without dst)
    with pytest.raises(ValueError):
        h.sample_plans(mean, sigma, (0, 1), Kn, dt=DT, src=pool)
    # straight through the C ABI: a null dst, actions given, candidates != groups * samples
    lib.mev_last_error.restype = ctypes.c_char_p
    roots, slots = np.array([0, 1], np.int32), np.array([2, 3, 4, 5], np.int32)
    ret = np.zeros((4, N), np.float32)

    def raw(**kw):
        xa = cap.MevSampleExpandArgs()
        sa = xa.sample
        sa.eval.roots, sa.eval.candidates, sa.eval.length, sa.eval.dt = cap._ptr(roots), 4, Tn, DT
        sa.eval.returns = cap._ptr(ret)
        sa.mean, sa.sigma, sa.groups, sa.samples = cap._ptr(mean), cap._ptr(sigma), Gn, Kn
        sa.lo, sa.hi = (ctypes.c_float * 2)(*LO), (ctypes.c_float * 2)(*HI)
        xa.dst, xa.dst_slots = pool._p, cap._ptr(slots)
        for k, v in kw.items():
            setattr(sa.eval if k in ("actions", "candidates") else sa if k in ("mean", "groups", "samples") else xa, k, v)
        return lib.mev_sample_expand_plans(h._h, ctypes.byref(xa)), lib.mev_last_error()

    assert raw(dst=None)[0] == -1 and b"dst and dst_slots required" in raw(dst=None)[1]
    rc, msg = raw(actions=cap._ptr(np.zeros((Tn, 4, N, 2), np.float32)))
    assert rc == -1 and b"mev_sample_expand_plans draws the actions" in msg
    for bad in (dict(candidates=5), dict(groups=0), dict(samples=3)):
        rc, msg = raw(**bad)
        assert rc == -1 and b"groups * samples" in msg, bad
    assert raw(mean=None)[0] == -1
    # nothing changed: the handle, and every slot of the pool
    EP._assert_same("refused calls", before, EP._snap_all(h))
    pa = pool.get_state(every)
    for name in pb[0]:
        assert G.bits_equal(pb[0][name], pa[0][name]), name
    assert pa[2].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and G.bits_equal(pb[1][0], pa[1][0])
    # valid calls work after the refused ones: through the C ABI, and with src == dst, an entry not stored
    assert raw()[0] == 0
    assert pool.get_state(every)[2].tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    out = call(src=pool, dst_slots=(-1, 6, 7, -1))
    assert pool.get_state(every)[2].tolist() == [1] * 8 and (out["substeps"] == Tn).all()
    other.close()
    h.close()


# 11
def _beam_search(mev, backend):
    """Two levels of a beam search over sampled plans: sample into pool_a, rank, continue the M elites
    of every group from their slots into pool_b."""
    import pkgload
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    En, N, Tn, Gn, M = 4, 2, 3, 3, 2
    v = vec_env.VecIntersectionEnv(En, N, lidar_rays=RAYS, use_team_reward=True, max_steps=10, backend=backend)
    RR.set_routes(v.handle)
    rng = np.random.default_rng(9)
    for t in range(4):
        v.step(RR.draw(rng, En, N, 0.6)[0])
    state = {k: x.copy() for k, x in v.handle.get_state().items()}
    C1, G2 = Gn * K, Gn * M
    C2 = G2 * K
    pool_a, pool_b, ref = v.make_pool(C1), v.make_pool(C2), v.make_pool(C2)
    roots = np.array([2, 0, 2], np.int32)
    mean, sigma = SP.draw_dist(N, groups=Gn, t=Tn)
    kw = dict(dt=DT, gamma=0.9, lo=LO, hi=HI, seed=SEED, copy=True)
    l1 = v.sample_plans(mean, sigma, roots, K, counter=5, dst=pool_a, dst_slots=np.arange(C1, dtype=np.int32), **kw)
    new = v.update_plans(l1["actions_out"], K, returns=l1["returns"], mode="elites", elites=M, sigma_min=0.05)
    order = new["order"].reshape(-1)  # the elites' candidate indices: their slots in pool_a
    if backend == "torch":
        m2, s2 = (new[k].repeat_interleave(M, dim=1) for k in ("new_mean", "new_sigma"))
    else:
        m2, s2 = (np.repeat(new[k], M, axis=1) for k in ("new_mean", "new_sigma"))
    l2 = v.sample_plans(m2, s2, order, K, counter=6, leaf_obs=True, src=pool_a, dst=pool_b,
                        dst_slots=np.arange(C2, dtype=np.int32), counter_offset=Tn, **kw)
    assert set(l2) == set(ALL) | {"leaf_obs", "actions_out"}
    if backend == "torch":
        order = order.cpu().numpy()
    x2 = v.expand_plans(l2["actions_out"], np.repeat(order, K).astype(np.int32), ref, np.arange(C2, dtype=np.int32),
                        src=pool_a, counter_offset=Tn, leaf_obs=True, dt=DT, gamma=0.9, copy=True)
    if backend == "torch":
        l1, new, l2, x2 = ({k: x.cpu().numpy() for k, x in d.items()} for d in (l1, new, l2, x2))
        m2, s2 = m2.cpu().numpy(), s2.cpu().numpy()
    assert G.bits_equal(l1["actions_out"], PN.sampled_actions(mean, sigma, K, LO, HI, SEED, 5))
    assert G.bits_equal(l2["actions_out"], PN.sampled_actions(m2, s2, K, LO, HI, SEED, 6))
    want = PN.elites(l1["actions_out"], PN.scores_of(l1["returns"]), K, M, 0.05)
    assert G.bits_equal(new["order"], want["order"])
    for k in OUT:
        assert G.bits_equal(l2[k], x2[k]), k
    same_slots("level 2", pool_b, np.arange(C2), ref, np.arange(C2))
    with pytest.raises(ValueError):
        v.sample_plans(mean, sigma, roots, K, src=pool_a)
    with pytest.raises(ValueError):
        v.sample_plans(mean, sigma, roots, K, dst_slots=np.arange(C1, dtype=np.int32))
    after = v.handle.get_state()
    for k in state:
        assert G.bits_equal(state[k], after[k]), k
    v.close()
    return dict(l1=l1, new=new, l2=l2)


def test_vec_env_beam_search(mev):
    a, b = _beam_search(mev, "numpy"), _beam_search(mev, "torch")
    for part in a:
        assert set(a[part]) == set(b[part])
        for k in a[part]:
            assert G.bits_equal(a[part][k], b[part][k]), f"{part}: {k}"
