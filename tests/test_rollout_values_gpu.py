"""mev_rollout_policy_values and mev_policy_set_value_head (include/marlenv.h), bit for bit.

Three handles with the same config, seed and history per case: A runs the new call, P runs mev_rollout_policy
with the same arguments, B runs actor_critic_ref.rollout_values_ref -- policy_ref's loop around the unchanged
Handle.step, the value head's FMA chain on the hidden activations of that loop, and one more forward pass on
the final observation.  value_seq must equal B's; every other output and the handle afterwards (state, last
outputs, diagnostics, snapshot bytes, three more steps) must equal both P's and B's."""
import ctypes

import numpy as np
import pytest

import actor_critic_ref as AC
import golden_replay as G
import policy_ref as PR
import test_evaluate_plans_gpu as EP
import test_rollout_policy_gpu as RP
import window_ref as RR
from window_ref import DT

pytestmark = pytest.mark.gpu

SEQS = RP.SEQS
WITH_VALUES = SEQS + ("value_seq",)


def head(H, seed, bias=0.3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(H) / np.sqrt(H)).astype(np.float32), np.array([bias], np.float32)


def triple(tag, mk, W, Bs, wv, bv, T, more=True, **kw):
    """The call on A, mev_rollout_policy on P, the defining loop on B; returns (out, ref, A's policy, (A, P, B))."""
    A, P, B = mk(), mk(), mk()
    pol = A.policy(W, Bs)
    assert not pol.has_value_head
    pol.set_value_head(wv, bv)
    assert pol.has_value_head
    out = A.rollout_policy(pol, T, outputs=WITH_VALUES, **kw)
    plain = P.rollout_policy(P.policy(W, Bs), T, **kw)
    ref = AC.rollout_values_ref(B, W, Bs, wv, bv, T, **kw)
    assert set(out) == set(WITH_VALUES) and out["value_seq"].shape == (T + 1, A.E, A.N)
    RP.assert_seqs(tag, out, ref, WITH_VALUES)
    RP.assert_seqs(tag + ": against mev_rollout_policy", out, plain, SEQS)
    RP.same_handles(tag + ": against mev_rollout_policy", A, P)
    RP.same_handles(tag, A, B)
    RP.conditions(tag, ref, T)
    v = ref["value_seq"]
    assert np.isfinite(v).all() and len(np.unique(v)) > 1, tag + ": the values do not vary"
    if more:
        RP.three_more_steps(tag + ": against mev_rollout_policy", A, P)
    return out, ref, pol, (A, P, B)


# ---- 1: every k_rollout row, the group loop with a partial second group, three policies, T = 1 and 5 ----

SHAPES = {
    "fixed row 3x8x64": (dict(E=3, N=8, rays=64, history=6, max_steps=2000), 3),
    "runtime row 5x3x16": (dict(E=5, N=3, rays=16, history=4, max_steps=2000), 0),
    "two groups 2x11x16": (dict(E=2, N=11, rays=16, history=4, max_steps=2000), 0),
    "traffic 32 slots 4x1x16": (dict(E=4, N=1, rays=16, history=30, traffic=True, density=20.0, max_npcs=32,
                                     max_steps=2000), 1),
    "traffic 64 slots 4x1x16": (dict(E=4, N=1, rays=16, history=30, traffic=True, density=20.0, max_npcs=64,
                                     max_steps=2000), 2),
}


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("hidden", [(64, 64), (128,), (5, 3)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_values_on_every_row(mev, shape, hidden, T):
    cfg, row = SHAPES[shape]
    cfg = dict(cfg)
    E, N, rays = cfg.pop("E"), cfg.pop("N"), cfg.pop("rays")
    mk = lambda: RP.make(mev, E, N, rays, **cfg)
    W, Bs = RP.net(127, hidden, 30 + len(hidden) + hidden[0])
    wv, bv = head(hidden[-1], 41)
    routes = [None]
    if cfg.get("traffic"):  # the Philox spawner, and replayed spawns
        routes.append(np.random.default_rng(31).integers(-1, 12, (T, E)))
    for route in routes:
        tag = f"{shape} {hidden} T={T}" + ("" if route is None else " spawn_route")
        kw = dict(dt=DT, auto_reset=bool(cfg.get("traffic")), spawn_route=route)
        out, ref, pol, hs = triple(tag, mk, W, Bs, wv, bv, T, **kw)
        assert hs[0].rollout_row() == row, tag
        if cfg.get("traffic") and T > 1:
            assert (ref["npc_count"] >= 1).any(), tag
        for h in hs:
            h.close()


# ---- 2: ends inside the window (max_steps = 3, auto-reset), noise, host and device pointers ----

def test_ends_inside_the_window_host_and_device(mev):
    import torch
    torch.cuda.set_device(0)
    E, N, rays, T = 5, 3, 16, 7
    mk = lambda: RP.make(mev, E, N, rays, history=1, max_steps=3, respawn=True)
    W, Bs = RP.net(127, (16, 16), 51, steer=0.9)
    wv, bv = head(16, 52)
    kw = dict(dt=1.0, auto_reset=True, sigma=(0.3, 0.25), seed=0x5EED0123456789AB, counter=(3 << 32) | 11)
    out, ref, pol, hs = triple("case 2", mk, W, Bs, wv, bv, T, **kw)
    ended = (ref["terminated_seq"] | ref["truncated_seq"]) != 0
    assert ended[:-1].any(0).all() and (ref["truncated_seq"][:-1] != 0).any()  # every env is reset inside the window
    assert ended[:-1].sum(0).min() >= 2
    # row t + 1 of an env that ended at t: the value of the terminal observation, the row the next action reads
    t, e = np.argwhere(ended[:-1])[0]
    _, hid = PR.forward(W, Bs, ref["obs_seq"][t, e])
    assert G.bits_equal(out["value_seq"][t + 1, e], AC.value_head(wv, bv, hid[-1]))
    # device pointers: the same bits, and the last outputs are row T - 1 of the caller's arrays
    Ad = mk()
    dw = lambda ws: [torch.as_tensor(w).cuda() for w in ws]
    pd = Ad.policy(dw(W), dw(Bs), device=True)
    pd.set_value_head(torch.as_tensor(wv).cuda(), torch.as_tensor(bv).cuda(), device=True)
    od = Ad.rollout_policy(pd, T, outputs=WITH_VALUES, device=True, **kw)
    Ad.sync()
    assert all(o.is_cuda for o in od.values()) and tuple(od["value_seq"].shape) == (T + 1, E, N)
    RP.assert_seqs("case 2, device pointers", od, ref, WITH_VALUES)
    for k, v in Ad.get_outputs().items():
        assert G.bits_equal(v, RP.B_last(ref, k, v)), k
    RP.same_handles("case 2, device pointers", Ad, hs[2])
    for h in hs + (Ad,):
        h.close()


# ---- 3: subnormal activations reach the value ----

def test_subnormal_activations(mev):
    E, N, rays, T = 2, 2, 8, 3
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    W, Bs = RP.net(127, (16, 16), 16)
    W[0] = (W[0] * np.float32(1e-30)).astype(np.float32)
    Bs[0] = (Bs[0] * np.float32(1e-36)).astype(np.float32)
    W[1] = (W[1] * np.float32(1e-9)).astype(np.float32)
    Bs[1] = (np.abs(Bs[1]) * np.float32(1e-42)).astype(np.float32)
    W[2] = (W[2] * np.float32(1e38)).astype(np.float32)
    wv, bv = head(16, 53)
    wv = (wv * np.float32(1e38)).astype(np.float32)
    out, ref, _, hs = triple("case 3", mk, W, Bs, wv, bv, T, dt=DT)
    tiny = np.float32(2.0 ** -126)
    h2 = ref["hidden"][1]
    assert ((h2 > 0) & (h2 < tiny)).any()  # subnormal activations: a flush anywhere would change them
    assert (np.abs(ref["value_seq"] - bv[0]) > 0).any()  # ... and they reach the value
    for h in hs:
        h.close()


# ---- 4: obs_seq NULL (the rows read in place), composition ----

def test_rows_read_in_place(mev):
    E, N, rays = 3, 2, 8
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    A, B = mk(), mk()
    W, Bs = RP.net(127, (16, 16), 18)
    wv, bv = head(16, 54)
    pol = A.policy(W, Bs)
    pol.set_value_head(wv, bv)
    ref = AC.rollout_values_ref(B, W, Bs, wv, bv, 7, dt=DT)
    first = A.rollout_policy(pol, 3, dt=DT, outputs=("actions_seq", "value_seq"))
    assert set(first) == {"actions_seq", "value_seq"}
    only = A.rollout_policy(pol, 4, dt=DT, outputs=("value_seq",))
    assert G.bits_equal(first["actions_seq"], ref["actions_seq"][:3])
    assert G.bits_equal(first["value_seq"], ref["value_seq"][:4])  # (row 3 is the bootstrap row of the first call)
    assert G.bits_equal(only["value_seq"], ref["value_seq"][3:])
    RP.same_handles("case 4", A, B)
    A.close(), B.close()


# ---- 5: the head in stream order, mev_policy_update keeps it, detach ----

def test_head_updates(mev):
    import torch
    torch.cuda.set_device(0)
    E, N, rays, T = 3, 2, 8, 3
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    W0, B0 = RP.net(127, (16, 16), 19)
    W1, B1 = RP.net(127, (16, 16), 20)
    (v0, c0), (v1, c1) = head(16, 55), head(16, 56, bias=-0.7)
    Bh = mk()
    ref0 = AC.rollout_values_ref(Bh, W0, B0, v0, c0, T, dt=DT)      # trunk 0, head 0
    ref1 = AC.rollout_values_ref(Bh, W0, B0, v1, c1, T, dt=DT)      # trunk 0, head 1 (the second window)
    ref2 = AC.rollout_values_ref(Bh, W1, B1, v1, c1, T, dt=DT)      # trunk 1, head 1 (the third)
    assert not G.bits_equal(ref0["value_seq"][0], AC.value_head(v1, c1, ref0["hidden"][-1][0]))
    # host pointers
    A = mk()
    pol = A.policy(W0, B0)
    pol.set_value_head(v0, c0)
    o0 = A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES)
    pol.set_value_head(v1, c1)
    o1 = A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES)
    pol.update(W1, B1)  # the repack leaves the head's column alone
    assert pol.has_value_head
    o2 = A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES)
    RP.assert_seqs("case 5, head 0", o0, ref0, WITH_VALUES)
    RP.assert_seqs("case 5, head 1", o1, ref1, WITH_VALUES)
    RP.assert_seqs("case 5, after mev_policy_update", o2, ref2, WITH_VALUES)
    RP.same_handles("case 5", A, Bh)
    # device pointers, everything queued before anything is read: a rollout issued before a change runs the old head
    Ad = mk()
    dw = lambda ws: [torch.as_tensor(w).cuda() for w in ws]
    dv = lambda x: torch.as_tensor(x).cuda()
    w0, b0, w1, b1 = dw(W0), dw(B0), dw(W1), dw(B1)
    hv = [dv(x) for x in (v0, c0, v1, c1)]
    pd = Ad.policy(w0, b0, device=True)
    pd.set_value_head(hv[0], hv[1], device=True)
    d0 = Ad.rollout_policy(pd, T, dt=DT, outputs=WITH_VALUES, device=True)
    pd.set_value_head(hv[2], hv[3], device=True)
    d1 = Ad.rollout_policy(pd, T, dt=DT, outputs=WITH_VALUES, device=True)
    pd.update(w1, b1, device=True)
    d2 = Ad.rollout_policy(pd, T, dt=DT, outputs=WITH_VALUES, device=True)
    Ad.sync()
    RP.assert_seqs("case 5, device, head 0", d0, ref0, WITH_VALUES)
    RP.assert_seqs("case 5, device, head 1", d1, ref1, WITH_VALUES)
    RP.assert_seqs("case 5, device, after mev_policy_update", d2, ref2, WITH_VALUES)
    # detach: the value call is refused, the plain call runs on, and a head can be attached again
    snap = EP._snap_all(A)
    pol.set_value_head(None, None)
    assert not pol.has_value_head
    with pytest.raises(mev.MevError):
        A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES)
    EP._assert_same("case 5, refused after the detach", snap, EP._snap_all(A))
    ref3 = AC.rollout_values_ref(Bh, W1, B1, v0, c0, T, dt=DT)
    RP.assert_seqs("case 5, detached: the plain call", A.rollout_policy(pol, T, dt=DT), ref3, SEQS)
    ref4 = AC.rollout_values_ref(Bh, W1, B1, v0, c0, T, dt=DT)
    pol.set_value_head(v0.reshape(1, -1), c0)  # (nn.Linear(H, 1).weight's shape)
    RP.assert_seqs("case 5, attached again", A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES), ref4, WITH_VALUES)
    with pytest.raises(ValueError):
        pol.set_value_head(np.zeros(15, np.float32), c0)
    with pytest.raises(mev.MevError):
        pol.set_value_head(np.full(16, np.nan, np.float32), c0)
    with pytest.raises(mev.MevError):
        pol.set_value_head(v0, np.array([np.inf], np.float32))
    ref5 = AC.rollout_values_ref(Bh, W1, B1, v0, c0, T, dt=DT)  # the refused heads changed nothing
    RP.assert_seqs("case 5, after refused heads", A.rollout_policy(pol, T, dt=DT, outputs=WITH_VALUES), ref5, WITH_VALUES)
    for h in (A, Ad, Bh):
        h.close()


# ---- 6: refused calls leave the handle untouched ----

def test_errors(mev):
    cap, lib = mev._capi, mev.load_library()
    E, N, rays = 2, 2, 8
    h = RP.make(mev, E, N, rays, history=3, max_steps=2000)
    other = RP.make(mev, E, N, rays)
    W, Bs = RP.net(h.D, (16, 16), 21)
    wv, bv = head(16, 57)
    pol, foreign, bare = h.policy(W, Bs), other.policy(W, Bs), h.policy(W, Bs)
    pol.set_value_head(wv, bv)
    foreign.set_value_head(wv, bv)
    ok = dict(dt=DT, outputs=WITH_VALUES)
    h.rollout_policy(pol, 2, **ok)
    mid = EP._snap_all(h)
    bad = [dict(T=0), dict(T=cap.MEV_MAX_ROLLOUT + 1), dict(flags=cap.MEV_GATHER_TO_ROOT), dict(flags=0x100),
           dict(lo=(0.5, -1.0), hi=(0.4, 1.0)), dict(hi=(np.inf, 1.0)), dict(lo=(np.nan, -1.0)), dict(sigma=(np.nan, 0.1)),
           dict(policy=foreign), dict(policy=None), dict(policy=bare)]
    for kw in bad:
        args = dict(ok, policy=pol, T=2)
        args.update(kw)
        with pytest.raises(mev.MevError):
            h.rollout_policy(args.pop("policy"), args.pop("T"), **args)
    # a null value_seq, straight at the C boundary
    va = cap.MevRolloutValuesArgs()
    va.rollout.policy, va.rollout.length, va.rollout.dt = pol._p, 2, DT
    va.rollout.lo = (ctypes.c_float * 2)(-1.0, -1.0)
    va.rollout.hi = (ctypes.c_float * 2)(1.0, 1.0)
    assert lib.mev_rollout_policy_values(h._h, ctypes.byref(va)) != 0
    assert lib.mev_rollout_policy_values(h._h, None) != 0
    EP._assert_same("refused calls", mid, EP._snap_all(h))
    # an unsupported shape: obs_dim above 31 + 128
    wide = mev.Handle(num_envs=2, num_agents=1, lidar_rays=8, obs_dim=31 + 129, device=0)
    wp = wide.policy(*RP.net(160, (8,), 1))
    wp.set_value_head(*head(8, 58))
    sw = EP._snap_all(wide)
    with pytest.raises(mev.MevError):
        wide.rollout_policy(wp, 2, **ok)
    EP._assert_same("unsupported shape", sw, EP._snap_all(wide))
    # after all that the call still runs, from where the refused ones left the handle: where it was
    twin = RP.make(mev, E, N, rays, history=3, max_steps=2000)
    AC.rollout_values_ref(twin, W, Bs, wv, bv, 2, dt=DT)
    r = AC.rollout_values_ref(twin, W, Bs, wv, bv, 2, dt=DT)
    RP.assert_seqs("after the refused calls", h.rollout_policy(pol, 2, **ok), r, WITH_VALUES)
    for x in (h, other, twin, wide):
        x.close()


# ---- the vector env layer: make_policy(value=...), rollout with value_seq, gae, refresh ----

def _vec_layer(mev, backend):
    import pkgload
    import torch
    pkgload.load()
    from marl_traffic_intersection_amd import vec_env
    E, N, T = 3, 2, 7

    def mkv():
        v = vec_env.VecIntersectionEnv(E, N, lidar_rays=8, max_steps=3, backend=backend)
        RR.set_routes(v.handle)
        return v

    v, twin = mkv(), mkv()
    torch.manual_seed(3)
    nn = torch.nn
    mod = nn.Sequential(nn.Linear(v.obs_dim, 16), nn.ReLU(), nn.Linear(16, 16), nn.ReLU(), nn.Linear(16, 2))
    critic = nn.Linear(16, 1)
    with torch.no_grad():
        mod[4].bias.copy_(torch.tensor([0.6, 0.0]))
    if backend == "torch":
        mod, critic = mod.cuda(), critic.cuda()
    host = lambda x: x.detach().cpu().numpy().copy()
    arrays = lambda: ([host(mod[i].weight) for i in (0, 2, 4)], [host(mod[i].bias) for i in (0, 2, 4)],
                      host(critic.weight), host(critic.bias))
    pol = v.make_policy(mod, value=critic)
    assert pol.has_value_head
    outputs = mev._capi.ROLLOUT_OUTPUTS + ("value_seq",)
    for rnd in range(2):  # the second window starts after an env's end or not: ended_before
        out = v.rollout(pol, T, sigma=(0.2, 0.1), seed=9, counter=rnd, outputs=outputs, copy=True)
        assert set(out) == set(WITH_VALUES) | {"ended_before"}
        if backend == "torch":
            assert all(x.is_cuda for x in out.values())
        W, Bs, wv, bv = arrays()
        ref = AC.rollout_values_ref(twin.handle, W, Bs, wv, bv, T, sigma=(0.2, 0.1), seed=9, counter=rnd, auto_reset=True)
        RP.assert_seqs(f"vec env {backend} window {rnd}", out, ref, WITH_VALUES + ("ended_before",))
        assert (ref["truncated_seq"][:-1] != 0).any()
        g = v.gae(out, 0.99, 0.95)
        adv, ret, valid = AC.gae_ref(ref["reward_seq"], ref["value_seq"], ref["done_seq"], ref["terminated_seq"],
                                     ref["truncated_seq"], ref["ended_before"], 0.99, 0.95, True)
        assert set(g) == {"advantages", "returns", "valid"}
        RP.assert_seqs(f"vec env {backend} gae {rnd}", g, dict(advantages=adv, returns=ret, valid=valid),
                       ("advantages", "returns", "valid"))
        assert (valid == 0).any() and (valid == 1).any()
        with torch.no_grad():  # a training step's worth of change to trunk and head, pushed without a new policy
            mod[0].weight.mul_(0.5)
            critic.weight.mul_(-1.5)
            critic.bias.add_(0.25)
        pol.refresh()
    v.close(), twin.close()


def test_vec_env_numpy(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch(mev):
    import torch
    assert torch.cuda.is_available()
    _vec_layer(mev, "torch")
