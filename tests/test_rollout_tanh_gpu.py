"""Tanh activations in the rollout policies (include/marlenv.h: MEV_POLICY_HIDDEN_TANH, MEV_POLICY_OUT_TANH, tanh_c),
bit for bit against policy_act_ref's defining loop -- the numpy policy with the stated tanh_c (pinned to mev_tanh by
test_policy_act_ref.py) around the unchanged Handle.step / Handle.step_repeat.  Handle A runs the call, handle B,
with the same config, seed and history, the loop; afterwards every *_seq array, the last outputs, the whole state
and the snapshot bytes are compared, and (cases 1 to 3) both take three more steps, which pins the Philox counter.

The conditions that keep a case from passing vacuously are asserted on the reference's results."""
import ctypes

import numpy as np
import pytest

import golden_replay as G
import policy_act_ref as PA
import policy_ref as PR
import test_rollout_policy_gpu as RP
import window_ref as RR
from rollout_repeat_ref import ALL, ALL_VALUES, SEQS
from window_ref import DT

pytestmark = pytest.mark.gpu
F = np.float32


def tnet(D, hidden, seed, act="tanh", out="linear", steer=0.0, head=None):
    """RP.net's weights with activations; head: the scale of a value head's weights (None: no head)"""
    W, B = RP.net(D, hidden, seed, steer)
    net = dict(weights=W, biases=B, hidden=act, out=out)
    if head is not None:
        rng = np.random.default_rng(seed + 1000)
        net["wv"] = (head * rng.standard_normal(hidden[-1])).astype(F)
        net["bv"] = np.array([0.25], F)
    return net


def policy(h, net):
    pol = h.policy(net["weights"], net["biases"], hidden=net["hidden"], out=net["out"])
    assert pol.activations == (net["hidden"], net["out"])
    if "wv" in net:
        pol.set_value_head(net["wv"], net["bv"])
    return pol


def conditions(tag, net, ref):
    """The tanh is visible: hidden units below zero (a ReLU would have stored 0) and strictly inside (-1, 1); a
    squashed mean lies in [-1, 1] and the actions differ between decisions."""
    for l, hid in enumerate(ref["hidden"][0]):
        if net["hidden"] == "tanh":
            assert (hid < 0).any() and (hid > 0).any() and (np.abs(hid) <= 1).all(), f"{tag}: hidden layer {l}"
        else:
            assert (hid == 0).any() and (hid > 0).any(), f"{tag}: hidden layer {l}"
    if net["out"] == "tanh":
        assert (np.abs(ref["mean_seq"]) <= 1).all() and (np.abs(ref["mean_seq"]) > 0).any(), tag
    T = ref["actions_seq"].shape[0]
    if T > 1:
        assert not G.bits_equal(ref["actions_seq"][0], ref["actions_seq"][T - 1]), tag + ": the actions never change"


def pair(tag, A, B, net, T, n=None, keys=SEQS, more=True, **kw):
    """The call on A, the defining loop on B, everything compared.  Returns (out, ref, policy)."""
    pol = policy(A, net)
    out = A.rollout_policy(pol, T, repeat=n or 1, outputs=keys, **kw)
    ref = PA.rollout_act_ref(B, net, T, n=n, **kw)
    RP.assert_seqs(tag, out, ref, keys)
    RP.same_handles(tag, A, B)
    conditions(tag, net, ref)
    if more:
        RP.three_more_steps(tag, A, B)
    return out, ref, pol


# ---- 1: the runtime row: both activations with noise and clamp, two lane passes, resets inside the window ----

@pytest.mark.parametrize("hidden,out", [((5, 3), "tanh"), ((128,), "linear")])
def test_runtime_row(mev, hidden, out):
    E, N, rays, T = 3, 2, 8, 4
    # (an episode of 2 steps: every env is truncated and reset inside the window, as RP's case 1 reaches it)
    mk = lambda: RP.make(mev, E, N, rays, max_steps=2, respawn=True)
    A, B = mk(), mk()
    assert A.rollout_row() == 0
    net = tnet(A.D, hidden, 31, out=out, steer=0.4)
    kw = dict(dt=1.0, auto_reset=True, sigma=(0.3, 0.25), lo=(-0.2, -0.5), hi=(0.9, 0.45), seed=0x5EED0123456789AB,
              counter=(3 << 32) | 11)
    out_, ref, _ = pair(f"case 1 {hidden}", A, B, net, T, **kw)
    ended = (ref["terminated_seq"] | ref["truncated_seq"]) != 0
    assert ended[:-1].any(0).all()  # every env is reset inside the window
    a = ref["actions_seq"]
    assert (a == F(0.9)).any() or (a == F(-0.2)).any() or (a[..., 1] == F(0.45)).any() or (a[..., 1] == F(-0.5)).any()
    assert not G.bits_equal(ref["actions_seq"], ref["mean_seq"])  # noise or clamp moved the actions off mu
    A.close(), B.close()


# ---- 2: the compile-time row ----

def test_compile_time_row(mev):
    E, N, rays, T = 4, 8, 64, 6
    mk = lambda: RP.make(mev, E, N, rays, history=6, max_steps=2000)
    A, B = mk(), mk()
    assert A.rollout_row() == RP.ROW_FIXED == 3
    pair("case 2", A, B, tnet(A.D, (64, 64), 32), T, dt=DT)
    A.close(), B.close()


# ---- 3: the traffic row ----

def test_traffic_row(mev):
    E, N, rays, T = 4, 1, 16, 6
    mk = lambda: RP.make(mev, E, N, rays, history=30, traffic=True, density=20.0, max_npcs=32, max_steps=2000)
    A, B = mk(), mk()
    assert A.rollout_row() == 1
    pair("case 3", A, B, tnet(A.D, (16, 16), 33, out="tanh"), T, dt=DT, auto_reset=True)
    assert (B.get_state()["npc_count"] > 0).any()
    A.close(), B.close()


# ---- 4: every branch of tanh_c on the device, against mev_tanh's bits ----

def bits(x):
    return np.asarray(x, F).view(np.uint32)


def around(c):
    c = F(c)
    return [np.nextafter(c, F(0)), c, np.nextafter(c, F(np.inf))]


PROBES = np.array(
    [0.0, -0.0, 1e-45, -1e-40, 1e-20, -3e-5, 0.1, -0.3, 0.55, 1.0, -2.5, 5.0, 8.5, -9.5, 20.0, -77.0, 3e38, -3e38]
    + around(2.0 ** -12) + [-v for v in around(2.0 ** -12)] + around(0.5625) + [-v for v in around(0.5625)]
    + around(10.0) + around(9.0109) + around(0.8664), F)  # (0.8664: the range reduction's n goes from 2 to 3)


def test_every_branch_on_the_device(mev):
    tanh = mev._capi.tanh_c
    A = RP.make(mev, 1, 1, 8, max_steps=2000)
    D, H = A.D, len(PROBES)
    assert H % 3 == 0 and H <= 128
    # hidden tanh: W0 = 0, so unit j is tanh_c(b0[j]) -- the chain fmaf(0, x[k], b0[j]) returns the bias itself, except
    # that a -0.0f bias leaves it as +0.0f (the output probe below reaches tanh_c(-0.0f))
    W0 = np.zeros((H, D), F)
    pre = PR.layer(W0, PROBES, A.get_outputs()["obs"][0, 0])
    assert (bits(pre) == bits(PROBES))[PROBES != 0].all() and (pre[PROBES == 0] == 0).all()
    want = tanh(pre)
    # (the probes reach every form: the identity, the polynomial, the exponential, the exact 1 and both signs of each)
    assert (want == PROBES).any() and (np.abs(want) == 1).any() and ((np.abs(want) > 0.5) & (np.abs(want) < 1)).any()
    # Output row c and the value head select one unit each; the weights of the units not selected are zeros signed
    # so that every product is -0.0f, and the output biases are -0.0f: the chain is then the selected unit itself.
    sel = lambda j: np.where(np.arange(H) == j, F(1.0), np.where(np.signbit(want), F(0.0), F(-0.0))).astype(F)
    neg0 = F(-0.0)
    pol = None
    for c0 in range(0, H, 3):
        W1, b1 = np.stack([sel(c0), sel(c0 + 1)]), np.array([neg0, neg0], F)
        if pol is None:
            pol = A.policy([W0, W1], [PROBES, b1], hidden="tanh")
        else:
            pol.update([W0, W1], [PROBES, b1])  # (mev_policy_update keeps the activations)
        pol.set_value_head(sel(c0 + 2), np.array([neg0], F))
        out = A.rollout_policy(pol, 1, dt=DT, lo=(-2.0, -2.0), hi=(2.0, 2.0), outputs=SEQS + ("value_seq",))
        got = np.concatenate([out["mean_seq"].reshape(2), out["value_seq"][0].reshape(1)])
        assert bits(got).tolist() == bits(want[c0:c0 + 3]).tolist(), (PROBES[c0:c0 + 3], got, want[c0:c0 + 3])
    assert pol.activations == ("tanh", "linear")
    pol.close()
    # the output tanh: a one-unit identity trunk h = relu(p) = p, mu = tanh_c(+-p), the value head v = p / 2 unsquashed
    pol = None
    for p in PROBES[~np.signbit(PROBES)]:  # (p = +0.0f: mu[1] = tanh_c(fmaf(-1, +0, -0)) = tanh_c(-0.0f) = -0.0f)
        spec = ([np.zeros((1, D), F), np.array([[1.0], [-1.0]], F)], [np.array([p], F), np.array([neg0, neg0], F)])
        if pol is None:
            pol = A.policy(*spec, out="tanh")
            pol.set_value_head(np.array([0.5], F), np.array([neg0], F))
        else:
            pol.update(*spec)
        out = A.rollout_policy(pol, 1, dt=DT, outputs=SEQS + ("value_seq",))
        assert bits(out["mean_seq"].reshape(2)).tolist() == bits(tanh(np.array([p, -p], F))).tolist(), p
        assert bits(out["value_seq"][0]).reshape(-1).tolist() == [int(bits(F(0.5) * p))], p
    assert pol.activations == ("relu", "tanh")
    A.close()


# ---- 5: the value and the frame-skip instantiations; the value is never squashed ----

def test_value_and_repeat(mev):
    E, N, rays, T, n = 3, 2, 8, 3, 2
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    A, B, A1, B1 = mk(), mk(), mk(), mk()
    net = tnet(A.D, (12, 7), 35, out="tanh", head=0.1)
    net["bv"] = np.array([3.0], F)  # (|wv . h| <= 0.1 * 7 * ~3 sigma with |h| < 1: every value lies above 1)
    kw = dict(dt=DT, sigma=(0.1, 0.2), seed=5, counter=9)
    out, ref, _ = pair("case 5 repeat", A, B, net, T, n=n, keys=ALL_VALUES, more=False, **kw)
    assert out["value_seq"].shape == (T + 1, E, N) and (ref["substeps_seq"] == n).all()
    assert (np.abs(ref["value_seq"]) > 1).any()  # not squashed (the mean is: conditions())
    assert not G.bits_equal(ref["value_seq"][T], ref["value_seq"][T - 1])  # row T is the bootstrap row's own
    # the plain value call (mev_rollout_policy_values) and the plain call, on their own instantiations
    keys = SEQS + ("value_seq",)
    out1, ref1, _ = pair("case 5 values", A1, B1, net, T, keys=keys, more=False, **kw)
    assert (np.abs(ref1["value_seq"]) > 1).any()
    pair("case 5 plain, after the value call", A1, B1, net, T, more=False, **kw)
    for h in (A, B, A1, B1):
        h.close()


# ---- 6: a ReLU and a tanh policy in one env ----

def test_multi_mixed_activations(mev):
    E, N, rays, T = 2, 3, 8, 3
    mk = lambda: RP.make(mev, E, N, rays, history=3, max_steps=2000)
    A, B = mk(), mk()
    nets = [tnet(A.D, (16,), 36, act="relu", head=1.0), tnet(A.D, (8, 6), 37, out="tanh", head=2.0)]
    assign = np.array([[0, 1, 0], [1, 1, 0]], np.uint8)
    sigma = [(0.1, 0.2), (0.3, 0.05)]
    kw = dict(dt=DT, seed=6, counter=2)
    out = A.rollout_policies([policy(A, x) for x in nets], assign, T, sigma=sigma, outputs=ALL_VALUES, **kw)
    ref = PA.rollout_act_ref(B, nets, T, n=1, assign=assign, sigma=sigma, **kw)
    RP.assert_seqs("case 6", out, ref, ALL_VALUES)
    RP.same_handles("case 6", A, B)
    # each slot's rows are its own policy's: the other policy's reference differs there
    for p in range(2):
        one = PA.policy_act_ref(nets[p], ref["obs_seq"][0], 1, sigma[p], seed=6, counter=2)[1]  # decision 1 reads row 0
        other = PA.policy_act_ref(nets[1 - p], ref["obs_seq"][0], 1, sigma[1 - p], seed=6, counter=2)[1]
        mine = assign == p
        assert G.bits_equal(out["mean_seq"][1][mine], one[mine])
        assert not G.bits_equal(out["mean_seq"][1][mine], other[mine])
    assert (ref["hidden"][0][0] == 0).any() and (ref["hidden"][1][0] < 0).any()  # a ReLU's zeros, a tanh's negatives
    A.close(), B.close()


# ---- 7: refusals, with the handle and the policy untouched ----

def test_refusals(mev):
    C = mev._capi
    lib = mev.load_library()
    mk = lambda: RP.make(mev, 2, 2, 8, history=2, max_steps=2000)
    A, B = mk(), mk()
    net = tnet(A.D, (6,), 38, out="tanh")
    pol = policy(A, net)
    plain = A.policy(net["weights"], net["biases"])
    flags = ctypes.c_uint32(99)
    assert lib.mev_policy_get_activations(plain._p, ctypes.byref(flags)) == 0 and flags.value == 0
    assert lib.mev_policy_get_activations(pol._p, ctypes.byref(flags)) == 0
    assert flags.value == C.MEV_POLICY_HIDDEN_TANH | C.MEV_POLICY_OUT_TANH == 0x30
    assert plain.activations == ("relu", "linear")
    assert lib.mev_policy_get_activations(None, ctypes.byref(flags)) == -1
    assert lib.mev_policy_get_activations(pol._p, None) == -1
    before = RP.EP._snap_all(A)
    other = [(2 * w).astype(F) for w in net["weights"]]
    spec, _keep = pol._spec(other, net["biases"], False)
    for bad in (C.MEV_POLICY_HIDDEN_TANH, C.MEV_POLICY_OUT_TANH, 0x30, 0x11, 0x40):  # an activation bit, an unknown bit
        assert lib.mev_policy_update(pol._p, ctypes.byref(spec), bad) == -1, hex(bad)
        assert lib.mev_policy_update(plain._p, ctypes.byref(spec), bad) == -1, hex(bad)
    h = ctypes.c_void_p()
    for bad in (0x40, 0x8, 0x2, 0x50, 0x80000000):  # an unknown bit on create
        assert lib.mev_policy_create(A._h, ctypes.byref(spec), bad, ctypes.byref(h)) == -1 and not h.value, hex(bad)
    assert b"polic" in lib.mev_last_error()
    for bad in (dict(hidden="gelu"), dict(out="sigmoid")):
        with pytest.raises(ValueError):
            A.policy(net["weights"], net["biases"], **bad)
    RP.EP._assert_same("case 7: the handle", before, RP.EP._snap_all(A))
    assert pol.activations == ("tanh", "tanh")
    # the refused updates left the weights alone: the policy still runs the net it was made with
    out = A.rollout_policy(pol, 2, dt=DT)
    ref = PA.rollout_act_ref(B, net, 2, dt=DT)
    RP.assert_seqs("case 7", out, ref)
    RP.same_handles("case 7", A, B)
    A.close(), B.close()


# ---- 8: the vector env layer: make_policy from a tanh module, rollout, refresh ----

def _vec_layer(mev, backend):
    import torch
    vec_env = mev.vec_env
    E, N, T = 3, 2, 4

    def mkv():
        v = vec_env.VecIntersectionEnv(E, N, lidar_rays=8, max_steps=2000, backend=backend)
        RR.set_routes(v.handle)
        return v

    v, twin = mkv(), mkv()
    torch.manual_seed(4)
    nn = torch.nn
    mod = nn.Sequential(nn.Linear(v.obs_dim, 16), nn.Tanh(), nn.Linear(16, 2), nn.Tanh())
    if backend == "torch":
        mod = mod.cuda()
    net = lambda: dict(weights=[mod[i].weight.detach().cpu().numpy().copy() for i in (0, 2)],
                       biases=[mod[i].bias.detach().cpu().numpy().copy() for i in (0, 2)], hidden="tanh", out="tanh")
    pol = v.make_policy(mod)
    assert pol.activations == ("tanh", "tanh")
    out = v.rollout(pol, T, sigma=(0.2, 0.1), seed=9, counter=1, copy=True)
    if backend == "torch":
        assert all(x.is_cuda for x in out.values())
    ref = PA.rollout_act_ref(twin.handle, net(), T, sigma=(0.2, 0.1), seed=9, counter=1, auto_reset=True)
    RP.assert_seqs(f"vec env {backend}", out, ref)
    conditions(f"vec env {backend}", net(), ref)
    with torch.no_grad():  # a training step's worth of change, pushed without a new policy
        mod[0].weight.mul_(0.5)
        mod[2].bias.add_(torch.tensor([0.3, 0.2], device=mod[2].bias.device))
    pol.refresh()
    assert pol.activations == ("tanh", "tanh")
    out = v.rollout(pol, T, outputs=("actions_seq", "mean_seq", "obs_seq"))
    ref = PA.rollout_act_ref(twin.handle, net(), T, auto_reset=True)
    RP.assert_seqs(f"vec env {backend}, refreshed", out, ref, ("actions_seq", "mean_seq", "obs_seq"))
    # arrays take the two keywords; a module's own activations cannot be overridden, nor changed by a refresh
    arr = v.make_policy((net()["weights"], net()["biases"]), hidden="tanh", out="tanh")
    assert arr.activations == ("tanh", "tanh")
    assert v.make_policy((net()["weights"], net()["biases"])).activations == ("relu", "linear")
    with pytest.raises(ValueError):
        v.make_policy(mod, hidden="relu")
    with pytest.raises(ValueError):
        pol.refresh(nn.Sequential(nn.Linear(v.obs_dim, 16), nn.ReLU(), nn.Linear(16, 2)))
    with pytest.raises(ValueError, match="same at every hidden layer"):
        v.make_policy(nn.Sequential(nn.Linear(v.obs_dim, 8), nn.Tanh(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 2)))
    v.close(), twin.close()


def test_vec_env_numpy(mev):
    _vec_layer(mev, "numpy")


def test_vec_env_torch(mev):
    import torch
    assert torch.cuda.is_available()
    _vec_layer(mev, "torch")
