"""mev_rollout_policies (include/marlenv.h): a policy per agent slot in one rollout, checked bit for bit against the
loop it is defined as.  Handle A runs the call; handle B, with the same config, seed and history, runs
rollout_multi_ref.rollout_multi_ref -- every listed policy's numpy policy_ref (pinned to libm's fmaf by
test_policy_ref.py; the selection by test_rollout_multi_ref.py) around the unchanged Handle.step_repeat.  Compared:
every element of every *_seq array and of substeps_seq, the last outputs, the whole state, the car sizes, the
diagnostics, the snapshot bytes, and the outputs of one further plain step on both handles.

The conditions that keep a case from passing vacuously are asserted on the reference's data alone."""
import ctypes

import numpy as np
import pytest

import golden_replay as G
import policy_ref as PR
import rollout_multi_ref as RM
import rollout_repeat_ref as RRR
import test_evaluate_plans_gpu as EP
import test_rollout_policy_gpu as RP
import test_rollout_repeat_gpu as RRG
import test_rollout_values_gpu as RV
import window_ref as RR
from rollout_repeat_ref import ALL, ALL_VALUES, SEQS
from window_ref import DT

pytestmark = pytest.mark.gpu

MEV_E_INVALID, MEV_E_RANGE = -1, -4  # include/marlenv.h


def nets_of(D, hiddens, seed, steer=0.0):
    """One (weights, biases, wv, bv) per entry of `hiddens`, each from its own seed."""
    out = []
    for p, hidden in enumerate(hiddens):
        W, Bs = RP.net(D, hidden, seed + 7 * p, steer=steer)
        out.append((W, Bs) + RV.head(hidden[-1], seed + 7 * p + 3, bias=0.3 - 0.5 * p))
    return out


def policies(h, nets, heads=True, device=False):
    pols = []
    for W, Bs, wv, bv in nets:
        if device:
            import torch
            dv = lambda x: torch.as_tensor(x).cuda()
            pol = h.policy([dv(w) for w in W], [dv(b) for b in Bs], device=True)
            if heads:
                pol.set_value_head(dv(wv), dv(bv), device=True)
        else:
            pol = h.policy(W, Bs)
            if heads:
                pol.set_value_head(wv, bv)
        pols.append(pol)
    return pols


def assign_for(E, N, P, seed):
    """Seeded, then: env 0 is all policy 1 (the other policies are skipped there), and env 1 holds all P policies --
    in its first group, or with N > 8 in its partial second group, whose first group has only policies 0 and 1.
    N == 1: env e has policy e % P."""
    if N == 1:
        return (np.arange(E) % P).astype(np.uint8).reshape(E, 1)
    a = np.random.default_rng(seed).integers(0, P, (E, N)).astype(np.uint8)
    a[0] = 1
    if N > 8:
        a[1, :8] = np.arange(8) % 2
        a[1, 8:] = (np.arange(N - 8) + P - 1) % P
    else:
        a[1] = np.arange(N) % P
    return a


def groups(assign):
    """The sets of policies of every (env, group of 8 agents)."""
    return [set(row[g:g + 8].tolist()) for row in assign for g in range(0, assign.shape[1], 8)]


def one_more_step(tag, hs):
    RRG.one_more_step(tag, hs)


# ---- 1: every k_rollout row, three policies of different depth and width, n = 1 and 3, T = 1 and 4 ----

SHAPES = dict(RV.SHAPES)
SHAPES["runtime row 3x8x64, one car 55x24"] = (dict(E=3, N=8, rays=64, history=6, max_steps=2000, one_car=True), 0)
HIDDENS = ((64, 64), (128,), (5, 3))


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_row(mev, shape, n, T):
    cfg, row = SHAPES[shape]
    cfg = dict(cfg)
    E, N, rays = cfg.pop("E"), cfg.pop("N"), cfg.pop("rays")
    mk = lambda: RRG.make(mev, E, N, rays, **cfg)
    A, Av, B = mk(), mk(), mk()
    tag = f"{shape} n={n} T={T}"
    assert A.rollout_row() == row, tag
    P = len(HIDDENS)
    nets = nets_of(A.D, HIDDENS, 30)
    assign = assign_for(E, N, P, 17)
    # the assignment reaches every path: asserted on the array the reference runs on
    gs = groups(assign)
    assert set(assign.reshape(-1)) == set(range(P)), tag + ": a policy drives no agent"
    if N == 1:
        assert len(set(assign[:, 0].tolist())) > 1, tag + ": the envs do not differ in policy"
    else:
        assert any(len(set(r.tolist())) == 1 for r in assign), tag + ": no env with exactly one policy"
        assert any(g == set(range(P)) for g in gs), tag + ": no group mixes all the policies"
    if N > 8:
        per_env = [gs[2 * e:2 * e + 2] for e in range(E)]
        assert any(g2 - g1 for g1, g2 in per_env), tag + ": no second group with a policy of its own"
    obs0 = B.get_outputs()["obs"].copy()
    kw = dict(dt=DT, auto_reset=bool(cfg.get("traffic")))
    ref = RM.rollout_multi_ref(B, nets, assign, T, n, **kw)
    out = A.rollout_policies(policies(A, nets, heads=False), assign, T, repeat=n, outputs=ALL, **kw)
    outv = Av.rollout_policies(policies(Av, nets), assign, T, repeat=n, outputs=ALL_VALUES, **kw)
    assert set(out) == set(ALL) and set(outv) == set(ALL_VALUES)
    RRR.assert_all(tag, out, ref, ALL)
    RRR.assert_all(tag + " with value_seq", outv, ref, ALL_VALUES)
    for name, h in (("", A), (" with value_seq", Av)):
        RP.same_handles(tag + name, h, B)  # get_state, get_outputs, get_car_dims, diagnostics, snapshot bytes
        RRG.last_outputs(tag + name, h, ref)
    # the same observation under two policies gives two different means: a slot driven by the wrong policy shows
    mus = [PR.forward(net[0], net[1], obs0)[0] for net in nets]
    for p in range(P):
        for q in range(p + 1, P):
            assert (mus[p].view(np.uint32) != mus[q].view(np.uint32)).any(-1).all(), f"{tag}: policies {p} and {q}"
    assert G.bits_equal(ref["mean_seq"][0], RM.select(assign, mus)), tag
    for p, layers in enumerate(ref["hidden"]):
        for l, hid in enumerate(layers):
            assert (hid == 0).any() and (hid > 0).any(), f"{tag}: policy {p} hidden layer {l}"
    if T > 1:
        assert not G.bits_equal(ref["actions_seq"][0], ref["actions_seq"][T - 1]), tag + ": the actions never change"
    assert (ref["substeps_seq"] >= 1).all() and (ref["substeps_seq"] == n).any(), tag
    v = ref["value_seq"]
    assert np.isfinite(v).all() and len(np.unique(v)) > 1, tag + ": the values do not vary"
    if cfg.get("traffic") and T > 1:
        assert (ref["npc_count"] >= 1).any(), tag
    one_more_step(tag, (A, Av, B))
    for h in (A, Av, B):
        h.close()


# ---- 2: one policy and assign all zero is the existing call ----

@pytest.mark.parametrize("shape", ["fixed row 3x8x64", "traffic 32 slots 4x1x16"])
def test_one_policy_is_the_existing_call(mev, shape):
    cfg, _ = SHAPES[shape]
    cfg = dict(cfg)
    E, N, rays, T = cfg.pop("E"), cfg.pop("N"), cfg.pop("rays"), 5
    hs = [RRG.make(mev, E, N, rays, **cfg) for _ in range(6)]
    snaps = [h.snapshot() for h in hs]
    assert all(G.bits_equal(snaps[0], s) for s in snaps[1:])  # twins
    W, Bs = RP.net(hs[0].D, (16, 16), 61)
    wv, bv = RV.head(16, 62)
    pols = [h.policy(W, Bs) for h in hs]
    for k in (0, 1, 2, 3):
        pols[k].set_value_head(wv, bv)
    zero = np.zeros((E, N), np.uint8)
    kw = dict(dt=DT, auto_reset=bool(cfg.get("traffic")), seed=5, counter=9)
    sig = (0.2, 0.1)
    m3 = hs[0].rollout_policies([pols[0]], zero, T, repeat=3, outputs=ALL_VALUES, sigma=[sig], **kw)
    r3 = hs[1].rollout_policy(pols[1], T, repeat=3, outputs=ALL_VALUES, sigma=sig, **kw)
    m1v = hs[2].rollout_policies([pols[2]], zero, T, outputs=ALL_VALUES, sigma=[sig], **kw)
    r1v = hs[3].rollout_policy(pols[3], T, outputs=SEQS + ("value_seq",), sigma=sig, **kw)
    m1 = hs[4].rollout_policies([pols[4]], zero, T, sigma=[sig], **kw)
    r1 = hs[5].rollout_policy(pols[5], T, sigma=sig, **kw)
    RRR.assert_all(shape + ": against mev_rollout_policy_repeat, n = 3", m3, r3, ALL_VALUES)
    RRR.assert_all(shape + ": against mev_rollout_policy_values", m1v, r1v, SEQS + ("value_seq",))
    RRR.assert_all(shape + ": against mev_rollout_policy", m1, r1, SEQS)
    assert set(m1) == set(SEQS) and (m1v["substeps_seq"] == 1).all()
    for a, b in ((0, 1), (2, 3), (4, 5)):
        RP.same_handles(f"{shape}: handles {a} and {b}", hs[a], hs[b])
    assert not G.bits_equal(r3["actions_seq"], r3["mean_seq"])  # (the noise is on)
    one_more_step(shape, hs[:2])
    one_more_step(shape, hs[2:])
    for h in hs:
        h.close()


# ---- 3 and 4: identical weights under any assignment; relabelling policies, sigma rows and assign ----

def test_identical_weights_are_the_single_policy_call(mev):
    E, N, rays, T, n = 3, 8, 64, 3, 2
    mk = lambda: RP.make(mev, E, N, rays, history=6, max_steps=2000)
    A, R = mk(), mk()
    net = nets_of(A.D, ((16, 16),), 71)[0]
    assign = np.random.default_rng(3).integers(0, 4, (E, N)).astype(np.uint8)
    assert all(len(g) > 1 for g in groups(assign)) and set(assign.reshape(-1)) == {0, 1, 2, 3}
    kw = dict(dt=DT, seed=11, counter=(1 << 32) | 2)
    out = A.rollout_policies(policies(A, [net] * 4), assign, T, repeat=n, outputs=ALL_VALUES, sigma=[(0.2, 0.1)] * 4, **kw)
    one = R.rollout_policy(policies(R, [net])[0], T, repeat=n, outputs=ALL_VALUES, sigma=(0.2, 0.1), **kw)
    RRR.assert_all("identical weights", out, one, ALL_VALUES)
    RP.same_handles("identical weights", A, R)
    A.close(), R.close()


def test_relabelling_gives_the_same_bits(mev):
    E, N, rays, T, n = 3, 8, 64, 3, 2
    mk = lambda: RP.make(mev, E, N, rays, history=6, max_steps=2000)
    A, R = mk(), mk()
    nets = nets_of(A.D, HIDDENS, 81)
    sigma = np.array([(0.3, 0.25), (0.0, 0.0), (0.1, 0.6)], np.float32)
    assign = assign_for(E, N, 3, 5)
    perm = np.array([2, 0, 1])  # new index q holds old policy perm[q]
    inv = np.argsort(perm).astype(np.uint8)
    kw = dict(dt=DT, seed=12, counter=4, repeat=n, outputs=ALL_VALUES)
    a = A.rollout_policies(policies(A, nets), assign, T, sigma=sigma, **kw)
    r = R.rollout_policies(policies(R, [nets[p] for p in perm]), inv[assign], T, sigma=sigma[perm], **kw)
    RRR.assert_all("relabelled", r, a, ALL_VALUES)
    RP.same_handles("relabelled", A, R)
    rows = [a["mean_seq"][0][assign == p] for p in range(3)]
    assert all(len(x) for x in rows) and not G.bits_equal(a["actions_seq"], a["mean_seq"])
    A.close(), R.close()


# ---- 5: per-policy noise, ends inside a window, auto-reset on and off; host and device pointers ----

CASE5 = dict(E=3, N=8, rays=64, n=4, T=5, dt=1.0, sigma=((0.3, 0.25), (0.0, 0.0)), seed=0x5EED0123456789AB,
             counter=(3 << 32) | 11)


@pytest.fixture(scope="module")
def case5(mev):
    C = CASE5
    mk = lambda: RRG.make(mev, C["E"], C["N"], C["rays"], history=1, max_steps=5, respawn=True)
    nets = nets_of(127, ((16, 16), (24,)), 51, steer=0.9)
    assign = assign_for(C["E"], C["N"], 2, 9)
    kw = dict(dt=C["dt"], sigma=C["sigma"], seed=C["seed"], counter=C["counter"])
    refs = {}
    for auto in (True, False):
        B = mk()
        refs[auto] = RM.rollout_multi_ref(B, nets, assign, C["T"], C["n"], auto_reset=auto, **kw)
        refs[auto]["handle"] = B
    yield dict(mk=mk, nets=nets, assign=assign, kw=kw, refs=refs)
    for r in refs.values():
        r["handle"].close()


def test_case5_conditions_on_the_reference(case5):
    ref, n, assign = case5["refs"][True], CASE5["n"], case5["assign"]
    k = ref["substeps_seq"]
    assert (k < n).any() and (k == n).any()  # windows cut short and windows that run out
    assert (ref["truncated_seq"][:-1] != 0).any() and (ref["done_seq"] != 0).any()  # an env ends inside; an agent is done
    assert ref["reset_first"][1:].any()  # a decision that begins with an auto-reset: the slot keeps its policy
    quiet = assign == 1  # sigma row (0, 0): action = clamp(mu); the other row is noisy
    a, mu = ref["actions_seq"], ref["mean_seq"]
    assert quiet.any() and (~quiet).any()
    assert G.bits_equal(a[:, quiet], np.clip(mu[:, quiet], np.float32(-1), np.float32(1)))
    assert (a[:, ~quiet] != np.clip(mu[:, ~quiet], np.float32(-1), np.float32(1))).any()
    off = case5["refs"][False]
    assert (off["truncated_seq"][1:] != 0).all() and not off["reset_first"].any()


@pytest.mark.parametrize("auto", [True, False])
def test_case5_host_and_device(mev, case5, auto):
    import torch
    torch.cuda.set_device(0)
    C, S = CASE5, case5
    ref, B = S["refs"][auto], S["refs"][auto]["handle"]
    tag = f"case 5 auto_reset={auto}"
    A = S["mk"]()
    out = A.rollout_policies(policies(A, S["nets"]), S["assign"], C["T"], repeat=C["n"], outputs=ALL_VALUES,
                             auto_reset=auto, **S["kw"])
    RRR.assert_all(tag, out, ref, ALL_VALUES)
    RP.same_handles(tag, A, B)
    Ad = S["mk"]()
    od = Ad.rollout_policies(policies(Ad, S["nets"], device=True), torch.as_tensor(S["assign"]).cuda(), C["T"],
                             repeat=C["n"], outputs=ALL_VALUES, device=True, auto_reset=auto, **S["kw"])
    Ad.sync()
    assert all(o.is_cuda for o in od.values()) and od["substeps_seq"].dtype == torch.int32
    RRR.assert_all(tag + ", device pointers", od, ref, ALL_VALUES)
    RRG.last_outputs(tag + ", device pointers", Ad, ref)  # (row T - 1 of the caller's arrays)
    RP.same_handles(tag + ", device pointers", Ad, B)
    A.close(), Ad.close()


# ---- 6: each output absent in turn ----

@pytest.fixture(scope="module")
def case6(mev):
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: RRG.make(mev, E, N, rays, history=3, max_steps=4, respawn=True)
    nets = nets_of(127, ((16, 16), (8,)), 18)
    assign = np.array([[0, 1], [1, 1], [1, 0]], np.uint8)
    B = mk()
    kw = dict(dt=DT, auto_reset=True, sigma=((0.2, 0.1), (0.05, 0.3)), seed=4, counter=2)
    ref = RM.rollout_multi_ref(B, nets, assign, T, n, **kw)
    assert (ref["substeps_seq"] < n).any() and (ref["substeps_seq"] == n).any()
    yield dict(mk=mk, nets=nets, assign=assign, T=T, n=n, kw=kw, ref=ref, B=B)
    B.close()


@pytest.mark.parametrize("absent", ALL_VALUES)
def test_each_output_absent_in_turn(case6, absent):
    S = case6
    A = S["mk"]()
    keys = tuple(k for k in ALL_VALUES if k != absent)
    out = A.rollout_policies(policies(A, S["nets"]), S["assign"], S["T"], repeat=S["n"], outputs=keys, **S["kw"])
    assert set(out) == set(keys)
    RRR.assert_all(f"without {absent}", out, S["ref"], keys)  # (obs_seq absent: the policies read the rows in place)
    RRG.last_outputs(f"without {absent}", A, S["ref"])       # the handle's own buffers hold row T - 1
    RP.same_handles(f"without {absent}", A, S["B"])
    A.close()


# ---- 7: assign out of range ----

def test_assign_out_of_range(mev):
    import torch
    torch.cuda.set_device(0)
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    A, Ad, B = mk(), mk(), mk()
    nets = nets_of(127, ((16, 16), (8,)), 28)
    assign = np.array([[0, 1], [200, 0], [1, 2]], np.uint8)
    clamped = np.minimum(assign, 1).astype(np.uint8)
    assert (assign >= 2).any() and set(clamped.reshape(-1)) == {0, 1}
    before = EP._snap_all(A)
    with pytest.raises(mev._capi.IndexRangeError):
        A.rollout_policies(policies(A, nets), assign, T, repeat=n, outputs=ALL_VALUES, dt=DT)
    EP._assert_same("assign out of range, host pointers", before, EP._snap_all(A))
    ma = mev._capi.MevRolloutMultiArgs()  # straight at the C boundary: the return code
    pa = policies(A, nets)
    table = (ctypes.c_void_p * 2)(pa[0]._p, pa[1]._p)
    ma.base.rollout.length, ma.base.rollout.dt, ma.base.repeat = T, DT, n
    ma.base.rollout.lo = (ctypes.c_float * 2)(-1.0, -1.0)
    ma.base.rollout.hi = (ctypes.c_float * 2)(1.0, 1.0)
    ma.policies, ma.count = ctypes.cast(table, ctypes.POINTER(ctypes.c_void_p)), 2
    ma.assign = assign.ctypes.data
    assert mev.load_library().mev_rollout_policies(A._h, ctypes.byref(ma)) == MEV_E_RANGE
    EP._assert_same("assign out of range at the C boundary", before, EP._snap_all(A))
    ref = RM.rollout_multi_ref(B, nets, clamped, T, n, dt=DT)
    od = Ad.rollout_policies(policies(Ad, nets), torch.as_tensor(assign).cuda(), T, repeat=n, outputs=ALL_VALUES, dt=DT,
                             device=True)
    Ad.sync()
    RRR.assert_all("assign out of range, device pointers: read as count - 1", od, ref, ALL_VALUES)
    RP.same_handles("assign out of range, device pointers", Ad, B)
    # the policies on the slots in question differ, so the clamp shows
    mus = [PR.forward(net[0], net[1], ref["obs_seq"][0])[0] for net in nets]
    assert not G.bits_equal(mus[0][assign >= 2], mus[1][assign >= 2])
    ok = A.rollout_policies(policies(A, nets), clamped, T, repeat=n, outputs=ALL_VALUES, dt=DT)  # the refused handle runs on
    RRR.assert_all("after the refused calls", ok, ref, ALL_VALUES)
    for h in (A, Ad, B):
        h.close()


# ---- 8: refused calls leave the handle untouched ----

def test_refusals(mev):
    cap, lib = mev._capi, mev.load_library()
    E, N, rays = 2, 2, 8
    h = RP.make(mev, E, N, rays, history=3, max_steps=2000, traffic=True, density=20.0, max_npcs=32)
    other = RP.make(mev, E, N, rays)
    twin = RP.make(mev, E, N, rays, history=3, max_steps=2000, traffic=True, density=20.0, max_npcs=32)
    nets = nets_of(h.D, ((16, 16), (8,)), 21)
    pols, foreign = policies(h, nets), policies(other, nets)[0]
    bare = policies(h, nets[1:], heads=False)[0]  # policy 1's layers without its value head
    assign = np.array([[0, 1], [1, 0]], np.uint8)
    ok = dict(dt=DT, outputs=ALL_VALUES, repeat=2, auto_reset=True)
    first = h.rollout_policies(pols, assign, 2, **ok)
    mid = EP._snap_all(h)
    nine = pols + [pols[0]] * 7
    bad = [dict(repeat=0), dict(repeat=cap.MEV_MAX_REPEAT + 1), dict(T=241, repeat=17),  # T * n = 4097
           dict(T=0), dict(T=cap.MEV_MAX_ROLLOUT + 1, repeat=1, outputs=("substeps_seq",)),
           dict(flags=cap.MEV_GATHER_TO_ROOT), dict(flags=0x100), dict(lo=(0.5, -1.0), hi=(0.4, 1.0)),
           dict(hi=(np.inf, 1.0)), dict(lo=(np.nan, -1.0)),
           dict(policies=None), dict(assign=None), dict(policies=[]), dict(policies=nine, assign=assign),
           dict(policies=[pols[0], None]), dict(policies=[foreign, pols[1]]), dict(policies=[pols[0], bare]),
           dict(sigma=((0.1, 0.2), (np.nan, 0.1))), dict(sigma=((0.1, np.inf), (0.3, 0.1)))]
    assert len(nine) == cap.MEV_MAX_ROLLOUT_POLICIES + 1
    for kw in bad:
        args = dict(ok, policies=pols, assign=assign, T=2)
        args.update(kw)
        with pytest.raises(mev.MevError) as err:
            h.rollout_policies(args.pop("policies"), args.pop("assign"), args.pop("T"), **args)
        assert f"error {MEV_E_INVALID}:" in str(err.value), kw
        EP._assert_same(f"refused {kw}", mid, EP._snap_all(h))
    # a policy without a head is fine while value_seq is not asked for ... (checked at the end: it runs)
    # straight at the C boundary: base.rollout.policy and base.rollout.sigma must be NULL; null arguments
    ma = cap.MevRolloutMultiArgs()
    table = (ctypes.c_void_p * 2)(pols[0]._p, pols[1]._p)
    ma.base.rollout.length, ma.base.rollout.dt, ma.base.repeat = 2, DT, 2
    ma.base.rollout.lo = (ctypes.c_float * 2)(-1.0, -1.0)
    ma.base.rollout.hi = (ctypes.c_float * 2)(1.0, 1.0)
    ma.policies, ma.count = ctypes.cast(table, ctypes.POINTER(ctypes.c_void_p)), 2
    ma.assign = assign.ctypes.data
    sig = (ctypes.c_float * 2)(0.1, 0.1)
    ma.base.rollout.policy = pols[0]._p
    assert lib.mev_rollout_policies(h._h, ctypes.byref(ma)) == MEV_E_INVALID
    ma.base.rollout.policy = None
    ma.base.rollout.sigma = ctypes.cast(sig, ctypes.POINTER(ctypes.c_float))
    assert lib.mev_rollout_policies(h._h, ctypes.byref(ma)) == MEV_E_INVALID
    ma.base.rollout.sigma = None
    for count in (0, -1, 9):
        ma.count = count
        assert lib.mev_rollout_policies(h._h, ctypes.byref(ma)) == MEV_E_INVALID
    ma.count = 2
    assert lib.mev_rollout_policies(h._h, None) == MEV_E_INVALID
    assert lib.mev_rollout_policies(None, ctypes.byref(ma)) == MEV_E_INVALID
    EP._assert_same("refused calls at the C boundary", mid, EP._snap_all(h))
    # in_dim != obs_dim: refused where such a policy is made (a policy is opaque and a handle's obs_dim is fixed)
    with pytest.raises(mev.MevError) as err:
        h.policy(*RP.net(h.D - 1, (16, 16), 1))
    assert f"error {MEV_E_INVALID}:" in str(err.value)
    # an unsupported shape: obs_dim above 31 + 128
    wide = mev.Handle(num_envs=2, num_agents=1, lidar_rays=8, obs_dim=31 + 129, device=0)
    assert wide.rollout_row() == -1
    wp = wide.policy(*RP.net(160, (8,), 1))
    sw = EP._snap_all(wide)
    with pytest.raises(mev.MevError) as err:
        wide.rollout_policies([wp], np.zeros((2, 1), np.uint8), 2, dt=DT, repeat=2)
    assert f"error {MEV_E_INVALID}:" in str(err.value)
    EP._assert_same("unsupported shape", sw, EP._snap_all(wide))
    # after all that the call still runs from where the refused ones left the handle -- where it was: the twin's
    # second window, traffic's Philox spawner included (the counter did not move)
    r1 = RM.rollout_multi_ref(twin, nets, assign, 2, 2, dt=DT, auto_reset=True)
    RRR.assert_all("the first call", first, r1, ALL_VALUES)
    r2 = RM.rollout_multi_ref(twin, nets, assign, 2, 2, dt=DT, auto_reset=True)
    out = h.rollout_policies([pols[0], bare], assign, 2, dt=DT, repeat=2, auto_reset=True, outputs=ALL)
    RRR.assert_all("after the refused calls, a policy without a head and no value_seq", out, r2, ALL)
    assert (r2["npc_count"] >= 1).any()
    one_more_step("after the refused calls", (h, twin))
    for x in (h, other, twin, wide):
        x.close()


# ---- 9: a listed policy updated between two calls on one stream ----

def test_update_in_stream_order(mev):
    import torch
    torch.cuda.set_device(0)
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    Ad, B = mk(), mk()
    nets = nets_of(127, ((16, 16), (8,)), 91)
    newer = nets_of(127, ((16, 16),), 95)[0]
    assign = np.array([[0, 1], [1, 1], [1, 0]], np.uint8)
    ref0 = RM.rollout_multi_ref(B, nets, assign, T, n, dt=DT)
    ref1 = RM.rollout_multi_ref(B, [newer, nets[1]], assign, T, n, dt=DT)
    stale = PR.forward(nets[0][0], nets[0][1], ref0["obs_seq"][T - 1])[0]
    assert not G.bits_equal(stale[assign == 0], ref1["mean_seq"][0][assign == 0])  # the update shows in window 2
    pols = policies(Ad, nets, device=True)
    dv = lambda x: torch.as_tensor(x).cuda()
    w, b, wv, bv = [dv(x) for x in newer[0]], [dv(x) for x in newer[1]], dv(newer[2]), dv(newer[3])
    da = dv(assign)
    d0 = Ad.rollout_policies(pols, da, T, repeat=n, outputs=ALL_VALUES, dt=DT, device=True)
    pols[0].update(w, b, device=True)  # everything queued before anything is read
    pols[0].set_value_head(wv, bv, device=True)
    d1 = Ad.rollout_policies(pols, da, T, repeat=n, outputs=ALL_VALUES, dt=DT, device=True)
    Ad.sync()
    RRR.assert_all("the call before the update: the old weights", d0, ref0, ALL_VALUES)
    RRR.assert_all("the call after the update: the new weights, the other policy untouched", d1, ref1, ALL_VALUES)
    RP.same_handles("stream order", Ad, B)
    Ad.close(), B.close()


# ---- 10: the vector env layer: rollout(policy=[p0, p1], assign=...) with value_seq and substeps_seq, then gae ----

def _vec_layer(mev, backend):
    import pkgload
    import torch
    import actor_critic_ref as AC
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, T, n = 3, 8, 4, 3

    def mkv():
        v = vec_env.VecIntersectionEnv(E, N, lidar_rays=64, max_steps=7, backend=backend)
        RR.set_routes(v.handle)
        return v

    v, twin = mkv(), mkv()
    torch.manual_seed(3)
    nn = torch.nn
    host = lambda x: x.detach().cpu().numpy().copy()
    pols, nets = [], []
    for width in (16, 24):
        mod = nn.Sequential(nn.Linear(v.obs_dim, width), nn.ReLU(), nn.Linear(width, 16), nn.ReLU(), nn.Linear(16, 2))
        critic = nn.Linear(16, 1)
        with torch.no_grad():
            mod[4].bias.copy_(torch.tensor([0.6, 0.0]))
        if backend == "torch":
            mod, critic = mod.cuda(), critic.cuda()
        pols.append(v.make_policy(mod, value=critic))
        nets.append(([host(mod[i].weight) for i in (0, 2, 4)], [host(mod[i].bias) for i in (0, 2, 4)],
                     host(critic.weight), host(critic.bias)))
    seats = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.uint8)  # [N]: the same seats in every env
    outputs = mev._capi.ROLLOUT_OUTPUTS + ("value_seq", "substeps_seq")
    sigma = ((0.2, 0.1), (0.0, 0.0))
    out = v.rollout(pols, T, sigma=sigma, seed=9, counter=1, outputs=outputs, repeat=n, copy=True, assign=seats)
    assert set(out) == set(outputs) | {"ended_before"}
    if backend == "torch":
        assert all(x.is_cuda for x in out.values())
    full = np.ascontiguousarray(np.broadcast_to(seats, (E, N)))
    ref = RM.rollout_multi_ref(twin.handle, nets, full, T, n, sigma=sigma, seed=9, counter=1, auto_reset=True)
    RRR.assert_all(f"vec env {backend}", out, ref, ALL_VALUES + ("ended_before",))
    assert (ref["truncated_seq"][:-1] != 0).any() and (ref["substeps_seq"] < n).any()
    g = v.gae(out, 0.99, 0.95)
    adv, ret, valid = AC.gae_ref(ref["reward_seq"], ref["value_seq"], ref["done_seq"], ref["terminated_seq"],
                                 ref["truncated_seq"], ref["ended_before"], 0.99, 0.95, True)
    RRR.assert_all(f"vec env {backend} gae", g, dict(advantages=adv, returns=ret, valid=valid),
                   ("advantages", "returns", "valid"))
    assert (valid == 0).any() and (valid == 1).any()
    # [E, N] is taken as it is: the second window, from where the first left both
    out2 = v.rollout(pols, T, sigma=sigma, seed=9, counter=2, outputs=outputs, repeat=n, copy=True, assign=full)
    ref2 = RM.rollout_multi_ref(twin.handle, nets, full, T, n, sigma=sigma, seed=9, counter=2, auto_reset=True)
    RRR.assert_all(f"vec env {backend}, assign [E, N]", out2, ref2, ALL_VALUES + ("ended_before",))
    with pytest.raises(ValueError):
        v.rollout(pols, T, repeat=n)  # a list of policies without assign
    with pytest.raises(ValueError):
        v.rollout(pols[0], T, repeat=n, assign=seats)  # assign with a single policy
    v.close(), twin.close()


def test_vec_env_numpy(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch(mev):
    import torch
    assert torch.cuda.is_available()
    _vec_layer(mev, "torch")
