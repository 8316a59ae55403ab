"""numpy restatement of what include/marlenv.h states for mev_policy_* and mev_rollout_policy: the f32 FMA
chain of a dense layer, the ReLU, the noise and the clamp, and the loop of policy + `Handle.step` that
mev_rollout_policy is defined as (rollout_ref).

Python 3.10 has no math.fma, so fma32 builds the exactly rounded f32 fmaf from float64: a product of two
f32 is exact in float64 (48 bits), the sum with c is rounded once to 53 bits, and TwoSum tells whether and
in which direction that sum is inexact; an inexact sum whose last bit is even moves to its odd neighbour
(round to odd), after which the rounding to f32 -- 24 bits, or fewer for a subnormal -- is the rounding
of the exact value.  tests/test_policy_ref.py pins it to libm's fmaf."""
import ctypes
import ctypes.util

import numpy as np

import plan_noise_ref as PN


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise: float32 arrays in, float32 out, one rounding."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b  # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
        inexact = np.isfinite(s) & (err != 0.0)
        even = (np.asarray(s).view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf))
        s = np.where(inexact & even, odd, s)
        return s.astype(np.float32)


_libm = None


def fmaf_libm(a, b, c):
    """libm's fmaf through ctypes, elementwise over flat float32 arrays (the pin of fma32)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fmaf.restype = ctypes.c_float
        _libm.fmaf.argtypes = [ctypes.c_float] * 3
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (a, b, c)))
    out = np.empty(a.shape, np.float32)
    f = _libm.fmaf
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        flat[i] = f(x, y, z)
    return out


def layer(W, b, x, fma=fma32):
    """y[..., j] = b[j], then y = fmaf(W[j][k], x[..., k], y) for k ascending."""
    W, b, x = np.asarray(W, np.float32), np.asarray(b, np.float32), np.asarray(x, np.float32)
    y = np.broadcast_to(b, x.shape[:-1] + b.shape).astype(np.float32)
    for k in range(W.shape[1]):
        y = fma(W[:, k], x[..., k, None], y)
    return y


def relu(y):
    """y > 0 ? y : 0 (NaN and -0.0 give +0.0)"""
    return np.where(y > np.float32(0.0), y, np.float32(0.0)).astype(np.float32)


def forward(weights, biases, x, fma=fma32):
    """mu [..., 2] and the hidden activations after the ReLU, for observation rows x [..., D]."""
    hidden = []
    h = np.asarray(x, np.float32)
    for W, b in zip(weights[:-1], biases[:-1]):
        h = relu(layer(W, b, h, fma))
        hidden.append(h)
    return layer(weights[-1], biases[-1], h, fma), hidden


def act(mu, sigma, lo, hi, eps=None):
    """fminf(fmaxf(sigma ? mu + sigma * eps : mu, lo), hi): multiply, then add, each rounded to f32."""
    x = np.asarray(mu, np.float32)
    if sigma is not None:
        x = (x + (np.asarray(sigma, np.float32) * eps).astype(np.float32)).astype(np.float32)
    return np.minimum(np.maximum(x, np.asarray(lo, np.float32)), np.asarray(hi, np.float32)).astype(np.float32)


def policy_ref(weights, biases, obs, t, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0, counter=0):
    """(actions, mu, hidden) of sub-step t for obs [E][N][D]; the noise word of env e, agent i, sub-step t."""
    mu, hidden = forward(weights, biases, obs)
    eps = None
    if sigma is not None:
        e, i = np.meshgrid(np.arange(obs.shape[0]), np.arange(obs.shape[1]), indexing="ij")
        eps = PN.noise(seed, counter, e, i, t)
    return act(mu, sigma, lo, hi, eps), mu, hidden


def rollout_ref(handle, weights, biases, T, dt=1.0 / 60.0, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0,
                counter=0, auto_reset=False, spawn_route=None):
    """The loop mev_rollout_policy is defined as, on `handle` (which it steps): a dict of the *_seq arrays,
    plus `hidden` (per hidden layer, the activations of every sub-step [T][E][N][width]) and `npc_count`
    ([T][E], after each sub-step)."""
    E, N, D = handle.E, handle.N, handle.D
    seq = dict(obs_seq=np.zeros((T, E, N, D), np.float32), actions_seq=np.zeros((T, E, N, 2), np.float32),
               mean_seq=np.zeros((T, E, N, 2), np.float32), reward_seq=np.zeros((T, E, N), np.float32),
               done_seq=np.zeros((T, E, N), np.uint8), status_seq=np.zeros((T, E, N), np.uint8),
               terminated_seq=np.zeros((T, E), np.uint8), truncated_seq=np.zeros((T, E), np.uint8))
    hidden = [np.zeros((T, E, N, np.shape(W)[0]), np.float32) for W in weights[:-1]]
    npc_count = np.zeros((T, E), np.int32)
    obs = handle.get_outputs()["obs"]
    for t in range(T):
        a, mu, hid = policy_ref(weights, biases, obs, t, sigma, lo, hi, seed, counter)
        r = handle.step(a, dt, spawn_route=None if spawn_route is None else spawn_route[t], auto_reset=auto_reset)
        obs = r["obs"]
        seq["obs_seq"][t], seq["actions_seq"][t], seq["mean_seq"][t] = obs, a, mu
        seq["reward_seq"][t], seq["done_seq"][t], seq["status_seq"][t] = r["reward"], r["done"], r["status"]
        seq["terminated_seq"][t], seq["truncated_seq"][t] = r["terminated"], r["truncated"]
        for l, x in enumerate(hid):
            hidden[l][t] = x
        npc_count[t] = handle.get_state()["npc_count"]
    seq["hidden"], seq["npc_count"] = hidden, npc_count
    return seq
