"""numpy restatements of what include/marlenv.h states for mev_sample_plans and mev_update_plans:
Philox4x32-10 with all four words kept, the Irwin-Hall noise, the sampled and clamped actions, the
rank within a group, the ELITES refit (exact, f32 in the stated order) and the SOFTMAX refit from
given weights (float64, the reference the stated bounds are measured against)."""
import numpy as np

M32 = 0xFFFFFFFF
EPS_SCALE = np.float32(1.0 / np.sqrt(43690.0))  # bits 0x3b9cc4bf
FLT_MAX = np.float32(np.finfo(np.float32).max)


def philox4(c0, c1, c2, c3, seed):
    """mev_kernels.hip philox4(): ten rounds over the counter (c0, c1, c2, c3) with key (lo32(seed), hi32(seed)); all
    four words.  The counter words may be uint64 arrays (values below 2^32) of one shape."""
    k0, k1 = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    m = np.uint64(M32)
    s32 = np.uint64(32)
    x0, x1, x2, x3 = (np.asarray(c, np.uint64) & m for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x0, np.uint64(0xCD9E8D57) * x2
        y0 = (p1 >> s32) ^ x1 ^ k0
        y2 = (p0 >> s32) ^ x3 ^ k1
        x1, x3, x0, x2 = p1 & m, p0 & m, y0, y2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return x0, x1, x2, x3


def byte_sum(w):
    w = np.asarray(w, np.uint64)
    return sum((w >> np.uint64(8 * b)) & np.uint64(0xFF) for b in range(4)).astype(np.int64)


def noise(seed, counter, c, i, s):
    """eps [..., 2] (float32) for candidates c, agents i, sub-step rows s (broadcast against each other)."""
    w = philox4(counter & M32, (counter >> 32) & M32, np.asarray(c, np.uint64) * np.uint64(64) + np.asarray(i, np.uint64),
                s, seed)
    b = [byte_sum(w[0]) + byte_sum(w[1]), byte_sum(w[2]) + byte_sum(w[3])]
    return np.stack([(x.astype(np.float32) - np.float32(1020.0)) * EPS_SCALE for x in b], -1).astype(np.float32)


def sampled_actions(mean, sigma, samples, lo, hi, seed, counter, mean_first=False):
    """actions_out [T][G * samples][N][2] for mean, sigma [T][G][N][2]."""
    mean, sigma = np.asarray(mean, np.float32), np.asarray(sigma, np.float32)
    T, G, N, _ = mean.shape
    C = G * samples
    s, c, i = np.meshgrid(np.arange(T), np.arange(C), np.arange(N), indexing="ij")
    eps = noise(seed, counter, c, i, s)
    if mean_first:
        eps[:, ::samples] = np.float32(0.0)
    g = np.arange(C) // samples
    x = (mean[:, g] + (sigma[:, g] * eps).astype(np.float32)).astype(np.float32)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return np.minimum(np.maximum(x, lo), hi).astype(np.float32)


def scores_of(returns):
    """score[c] = the f32 sum of returns[c][i] over i = 0..N-1, in that order."""
    returns = np.asarray(returns, np.float32)
    sc = np.zeros(returns.shape[0], np.float32)
    for i in range(returns.shape[1]):
        sc = (sc + returns[:, i]).astype(np.float32)
    return sc


def keys_of(scores):
    """non-finite scores become -FLT_MAX"""
    k = np.asarray(scores, np.float32).copy()
    k[~np.isfinite(k)] = -FLT_MAX
    return k


def rank_order(keys):
    """j in rank order: the higher score first, equal scores (-0.0 == +0.0) by the lower j."""
    k = np.asarray(keys, np.float32) + np.float32(0.0)  # (-0.0 -> +0.0, so the stable sort sees them equal)
    return np.argsort(-k.astype(np.float64), kind="stable")


def elites(actions, scores, samples, M, sigma_min=0.0):
    """dict of new_mean, new_sigma [T][G][N][2], best, best_score [G], order [G][M]: the header's ELITES arithmetic."""
    a = np.asarray(actions, np.float32)
    T, C, N, _ = a.shape
    G = C // samples
    key = keys_of(scores).reshape(G, samples)
    mean, sig = np.zeros((T, G, N, 2), np.float32), np.zeros((T, G, N, 2), np.float32)
    order = np.zeros((G, M), np.int32)
    for g in range(G):
        order[g] = g * samples + rank_order(key[g])[:M]
        s = np.zeros((T, N, 2), np.float32)
        for c in order[g]:
            s = (s + a[:, c]).astype(np.float32)
        mu = (s / np.float32(M)).astype(np.float32)
        q = np.zeros((T, N, 2), np.float32)
        for c in order[g]:
            d = (a[:, c] - mu).astype(np.float32)
            q = (q + (d * d).astype(np.float32)).astype(np.float32)
        mean[:, g] = mu
        sig[:, g] = np.maximum(np.sqrt((q / np.float32(M)).astype(np.float32)).astype(np.float32), np.float32(sigma_min))
    return dict(new_mean=mean, new_sigma=sig, best=order[:, 0].copy(), best_score=key.reshape(-1)[order[:, 0]], order=order)


def softmax_x(scores, samples, inv_temperature):
    """The f32 exponent arguments x_j = (score_j - best) * inv_temperature, [G][samples], with best and best_score."""
    key = keys_of(scores)
    G = key.size // samples
    key = key.reshape(G, samples)
    first = np.array([rank_order(key[g])[0] for g in range(G)])
    top = key[np.arange(G), first]
    x = ((key - top[:, None]).astype(np.float32) * np.float32(inv_temperature)).astype(np.float32)
    return x, (np.arange(G) * samples + first).astype(np.int32), top


def softmax64(actions, x, samples):
    """The SOFTMAX refit in float64 from the f32 arguments x [G][samples]: mean, q (= sigma^2), weights, and
    A = max |a| over the group's candidates, each [T][G][N][2] (weights [C])."""
    a = np.asarray(actions, np.float64)
    T, C, N, _ = a.shape
    G = C // samples
    w = np.exp(np.asarray(x, np.float64))
    W = w.sum(1)
    ag = a.reshape(T, G, samples, N, 2)
    mean = np.einsum("gj,tgjik->tgik", w, ag) / W[None, :, None, None]
    d = ag - mean[:, :, None]
    q = np.einsum("gj,tgjik->tgik", w, d * d) / W[None, :, None, None]
    return dict(mean=mean, q=q, weights=(w / W[:, None]).reshape(-1), A=np.abs(ag).max(2))
