"""numpy restatement of what include/marlenv.h states for mev_policy_set_value_head,
mev_rollout_policy_values and mev_gae.

values_ref: the value rows of a rollout -- the head's FMA chain (policy_ref.layer) on the last hidden
activations policy_ref.rollout_ref already returns for sub-steps 0..T-1, plus one forward pass on the final
observation for row T.  rollout_values_ref: rollout_ref with value_seq and ended_before added.

gae_ref: the header's block line for line, a plain loop over f32 scalars: every product and every sum
is rounded to f32 where it stands (numpy float32 scalars do not fuse)."""
import numpy as np

import policy_ref as PR

F = np.float32


def value_head(wv, bv, h_last):
    """v = layer(wv, bv, h_last)[0] for activations [..., H_last]"""
    wv = np.asarray(wv, F).reshape(1, -1)
    bv = np.asarray(bv, F).reshape(1)
    return PR.layer(wv, bv, h_last)[..., 0]


def values_ref(weights, biases, wv, bv, ref):
    """value_seq [T + 1][E][N] of a rollout_ref result `ref`"""
    T = ref["obs_seq"].shape[0]
    out = np.zeros((T + 1,) + ref["obs_seq"].shape[1:3], F)
    out[:T] = value_head(wv, bv, ref["hidden"][-1])
    _, hid = PR.forward(weights, biases, ref["obs_seq"][T - 1])
    out[T] = value_head(wv, bv, hid[-1])
    return out


def rollout_values_ref(handle, weights, biases, wv, bv, T, **kw):
    """rollout_ref on `handle` (which it steps) plus value_seq, and ended_before [E] taken before the loop"""
    last = handle.get_outputs()
    ended = ((last["terminated"] != 0) | (last["truncated"] != 0)).astype(np.uint8)
    ref = PR.rollout_ref(handle, weights, biases, T, **kw)
    ref["value_seq"] = values_ref(weights, biases, wv, bv, ref)
    ref["ended_before"] = ended
    return ref


def gae_ref(reward, value, done=None, terminated=None, truncated=None, ended_before=None, gamma=0.99, lam=0.95,
            mask_reset_steps=False):
    """(advantages, returns, valid), each [T][E][N]"""
    r, V = np.asarray(reward, F), np.asarray(value, F)
    T, E, N = r.shape
    assert V.shape == (T + 1, E, N)
    gamma, lam = F(gamma), F(lam)
    c = F(gamma * lam)
    adv_out, ret_out, valid_out = np.zeros((T, E, N), F), np.zeros((T, E, N), F), np.zeros((T, E, N), np.uint8)
    for e in range(E):
        for i in range(N):
            adv_next = F(0.0)
            for t in range(T - 1, -1, -1):
                stop = bool(done is not None and done[t][e][i]) or bool(terminated is not None and terminated[t][e])
                cut = stop or bool(truncated is not None and truncated[t][e])
                nv = F(0.0) if stop else V[t + 1][e][i]
                delta = F(F(r[t][e][i] + F(gamma * nv)) - V[t][e][i])
                adv = delta if cut else F(delta + F(c * adv_next))
                valid = 1
                if mask_reset_steps:
                    if t > 0:
                        before = bool(terminated is not None and terminated[t - 1][e]) or \
                            bool(truncated is not None and truncated[t - 1][e])
                    else:
                        before = bool(ended_before is not None and ended_before[e])
                    if before:
                        adv, valid = F(0.0), 0
                ret = F(adv + V[t][e][i])
                adv_next = adv
                adv_out[t][e][i], ret_out[t][e][i], valid_out[t][e][i] = adv, ret, valid
    return adv_out, ret_out, valid_out


def gae_ref64(reward, value, done=None, terminated=None, truncated=None, ended_before=None, gamma=0.99, lam=0.95,
              mask_reset_steps=False):
    """The same recurrence in float64, vectorised over (e, i): a sanity check of gae_ref, not the contract."""
    r, V = np.asarray(reward, np.float64), np.asarray(value, np.float64)
    T, E, N = r.shape
    z = np.zeros((T, E), bool)
    d = np.zeros((T, E, N), bool) if done is None else np.asarray(done) != 0
    te = z if terminated is None else np.asarray(terminated) != 0
    tr = z if truncated is None else np.asarray(truncated) != 0
    eb = np.zeros(E, bool) if ended_before is None else np.asarray(ended_before) != 0
    g, c = float(F(gamma)), float(F(gamma)) * float(F(lam))
    adv = np.zeros((T, E, N))
    nxt = np.zeros((E, N))
    for t in range(T - 1, -1, -1):
        stop = d[t] | te[t][:, None]
        cut = stop | tr[t][:, None]
        delta = r[t] + g * np.where(stop, 0.0, V[t + 1]) - V[t]
        a = np.where(cut, delta, delta + c * nxt)
        if mask_reset_steps:
            before = (te[t - 1] | tr[t - 1]) if t > 0 else eb
            a = np.where(before[:, None], 0.0, a)
        adv[t] = nxt = a
    return adv, adv + V[:T]
