"""numpy restatement of what include/marlenv.h states for the policies' activations: tanh_c, written from the
header's text operation for operation (policy_ref.fma32 for every fmaf, numpy float32 for every other rounding),
the two activation rules, and the defining loops of the rollout calls with a net's activations as parameters.

A net is a dict: weights, biases, hidden ("relu" | "tanh"), out ("linear" | "tanh"), and optionally wv, bv (a value
head).  rollout_act_ref is ONE loop for all four calls: per decision every listed net's policy on the whole
observation (policy_ref.layer / act, plan_noise_ref.noise), the rows selected per slot by `assign`
(rollout_multi_ref.select), then the unchanged Handle.step (n None: the plain calls) or Handle.step_repeat; the
value rows are the head's chain on each net's own last hidden activations, never squashed.

tests/test_policy_act_ref.py pins tanh_c here to mev_tanh bit for bit.  Every comparison against these results is
on bits over every element."""
import numpy as np

import actor_critic_ref as AC
import plan_noise_ref as PN
import policy_ref as PR
from rollout_multi_ref import select

F = np.float32
_h = lambda s: F(float.fromhex(s))
Q = [_h(s) for s in ("-0x1.555554p-2", "0x1.110fbap-3", "-0x1.b9915ep-5", "0x1.5c6c6p-6", "-0x1.abecbp-8")]
LOG2E, LN2_HI, LN2_LO = _h("0x1.715476p+0"), _h("0x1.62e4p-1"), _h("0x1.7f7d1cp-20")
Gc = [_h(s) for s in ("0x1p-1", "0x1.5554dcp-3", "0x1.5554e8p-5", "0x1.120c74p-7", "0x1.6d445ep-10")]
TINY, SMALL, SAT = _h("0x1p-12"), F(0.5625), F(10.0)
# the values the sequence branches on: its thresholds, and where the exponential form first gives exactly 1
THRESHOLDS = (TINY, SMALL, SAT, F(9.0109))


def tanh_c(y):
    """The header's sequence, elementwise over a float32 array."""
    y = np.asarray(y, F)
    fma = PR.fma32
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(y)
        ac = np.where(a < SAT, a, SAT).astype(F)  # (NaN gives 10)
        s = (ac * ac).astype(F)
        q = fma(s, fma(s, fma(s, fma(s, Q[4], Q[3]), Q[2]), Q[1]), Q[0])
        p = fma((ac * s).astype(F), q, ac)
        x = (ac + ac).astype(F)
        n = np.rint((x * LOG2E).astype(F)).astype(F)  # (to nearest, ties to even)
        r = fma(-n, LN2_LO, fma(-n, LN2_HI, x))
        g = fma(r, fma(r, fma(r, fma(r, Gc[4], Gc[3]), Gc[2]), Gc[1]), Gc[0])
        scale = ((n.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F)
        E = (fma(r, fma(r, g, F(1.0)), F(1.0)) * scale).astype(F)
        t = (F(1.0) - (F(2.0) / (E + F(1.0)).astype(F)).astype(F)).astype(F)
        m = np.where(a < TINY, a, np.where(a < SMALL, p, t)).astype(F)
        signed = (m.view(np.uint32) | (y.view(np.uint32) & np.uint32(0x80000000))).view(F)
        return np.where(y != y, F(0.0), signed).astype(F)


def hidden_act(name):
    return {"relu": PR.relu, "tanh": tanh_c}[name]


def forward(net, x):
    """(mu [..., 2] -- squashed where the net says so -- and the hidden activations) for rows x [..., D]"""
    f = hidden_act(net.get("hidden", "relu"))
    hid = []
    h = np.asarray(x, F)
    for W, b in zip(net["weights"][:-1], net["biases"][:-1]):
        h = f(PR.layer(W, b, h))
        hid.append(h)
    mu = PR.layer(net["weights"][-1], net["biases"][-1], h)
    if net.get("out", "linear") == "tanh":
        mu = tanh_c(mu)
    return mu, hid


def forward64(net, x):
    """The same network in float64 with numpy's tanh: what the module itself computes, to rounding."""
    f = {"relu": lambda v: np.maximum(v, 0.0), "tanh": np.tanh}[net.get("hidden", "relu")]
    h = np.asarray(x, np.float64)
    for W, b in zip(net["weights"][:-1], net["biases"][:-1]):
        h = f(h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))
    mu = h @ np.asarray(net["weights"][-1], np.float64).T + np.asarray(net["biases"][-1], np.float64)
    return np.tanh(mu) if net.get("out", "linear") == "tanh" else mu


def policy_act_ref(net, obs, t, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0, counter=0):
    """(actions, mu, hidden) of decision t for obs [E][N][D]: noise and clamp follow the (squashed) mu unchanged"""
    mu, hid = forward(net, obs)
    eps = None
    if sigma is not None:
        e, i = np.meshgrid(np.arange(obs.shape[0]), np.arange(obs.shape[1]), indexing="ij")
        eps = PN.noise(seed, counter, e, i, t)
    return PR.act(mu, sigma, lo, hi, eps), mu, hid


def rollout_act_ref(handle, nets, T, n=None, assign=None, sigma=None, dt=1.0 / 60.0, lo=(-1.0, -1.0), hi=(1.0, 1.0),
                    seed=0, counter=0, auto_reset=False, spawn_route=None):
    """The defining loop on `handle` (which it steps).  nets: one net or a list; assign [E][N] (default: all 0);
    sigma: [2] for one net, [P][2] for a list; n: None for Handle.step, else Handle.step_repeat's n.  Returns the
    *_seq arrays (substeps_seq with n; value_seq where every net has a head), `hidden` [p][layer] and
    `ended_before`."""
    single = isinstance(nets, dict)
    if single:
        nets, sigma = [nets], None if sigma is None else [sigma]
    E, N, D = handle.E, handle.N, handle.D
    assign = np.zeros((E, N), np.uint8) if assign is None else np.asarray(assign, np.uint8)
    seq = dict(obs_seq=np.zeros((T, E, N, D), F), actions_seq=np.zeros((T, E, N, 2), F),
               mean_seq=np.zeros((T, E, N, 2), F), reward_seq=np.zeros((T, E, N), F),
               done_seq=np.zeros((T, E, N), np.uint8), status_seq=np.zeros((T, E, N), np.uint8),
               terminated_seq=np.zeros((T, E), np.uint8), truncated_seq=np.zeros((T, E), np.uint8))
    if n is not None:
        seq["substeps_seq"] = np.zeros((T, E), np.int32)
    hidden = [[np.zeros((T, E, N, np.shape(W)[0]), F) for W in net["weights"][:-1]] for net in nets]
    last = handle.get_outputs()
    seq["ended_before"] = ((last["terminated"] != 0) | (last["truncated"] != 0)).astype(np.uint8)
    obs = last["obs"]
    for t in range(T):
        per = [policy_act_ref(net, obs, t, None if sigma is None else sigma[p], lo, hi, seed, counter)
               for p, net in enumerate(nets)]
        a, mu = select(assign, [r[0] for r in per]), select(assign, [r[1] for r in per])
        sp = None if spawn_route is None else np.asarray(spawn_route)[t]
        if n is None:
            r = handle.step(a, dt, spawn_route=sp, auto_reset=auto_reset)
        else:
            r = handle.step_repeat(a, n, dt, spawn_route=sp, auto_reset=auto_reset)
            seq["substeps_seq"][t] = r["substeps"]
        obs = r["obs"].copy()
        seq["obs_seq"][t], seq["actions_seq"][t], seq["mean_seq"][t] = obs, a, mu
        seq["reward_seq"][t], seq["done_seq"][t], seq["status_seq"][t] = r["reward"], r["done"], r["status"]
        seq["terminated_seq"][t], seq["truncated_seq"][t] = r["terminated"], r["truncated"]
        for p, res in enumerate(per):
            for l, x in enumerate(res[2]):
                hidden[p][l][t] = x
    seq["hidden"] = hidden
    if all("wv" in net for net in nets):
        rows = []
        for p, net in enumerate(nets):
            v = np.zeros((T + 1, E, N), F)
            v[:T] = AC.value_head(net["wv"], net["bv"], hidden[p][-1])
            v[T] = AC.value_head(net["wv"], net["bv"], forward(net, seq["obs_seq"][T - 1])[1][-1])
            rows.append(v)
        seq["value_seq"] = select(np.broadcast_to(assign, (T + 1, E, N)), rows)
    return seq


def sweep_inputs(stride=40009):
    """The strided sweep and the threshold neighbourhoods of the CPU pin: every binade of finite f32 at a stride,
    both signs, 2^10 floats on either side of every value the sequence branches on, and the special values."""
    pos = np.arange(0, 0x7F800000, stride, dtype=np.uint32)
    near = np.concatenate([np.arange(int(np.asarray(c, F).view(np.uint32)) - 1024, int(np.asarray(c, F).view(np.uint32)) + 1025,
                                     dtype=np.int64).astype(np.uint32) for c in THRESHOLDS])
    sub = np.arange(0, 2048, dtype=np.uint32)
    special = np.array([0x7F800000, 0x7FC00000, 0x7F800001, 0x7F7FFFFF, 0x00800000, 0x007FFFFF], np.uint32)
    u = np.concatenate([pos, near, sub, special])
    return np.concatenate([u, u | np.uint32(0x80000000)]).view(F)
