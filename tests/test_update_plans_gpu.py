"""mev_update_plans (include/marlenv.h): the reduction over each group's candidates.  No simulation:
actions and scores are drawn with numpy on 2-env handles (N = 1 and N = 12).

ELITES is compared bit for bit with the numpy restatement (plan_noise_ref.elites); best, best_score
and order are exact in both modes.

SOFTMAX is compared with a float64 reference fed the same f32 exponent arguments x_j
(plan_noise_ref.softmax64).  The device's expf is HIP's, documented within 1 ulp; the bounds below
allow the 2 ulp the header's derivation assumes.  With u = 2^-23, K candidates per group and A =
max |a| over the group's candidates for that (s, i, k):

  weights: w_j / W carries expf's error twice (2 ulp each: 4 u), K roundings of the running sum W
      (K u / 2) and the division (u / 2):       |w - ref| <= (K + 8) u ref
  mean:    the numerator adds one rounding per product and K for its running sum, on terms
      bounded by w_j A:                         |mean - ref| <= (K + 8) u A       (the stated bound)
  q:       sum_j w_j (a_j - m)^2 / W = q_ref + (m - mean_ref)^2 for any m, so the device's mean
      enters in second order only: ((K + 8) u A)^2.  Each term has |d| <= 2 A, d itself one
      rounding (d^2: u), two products (u) against the mean's one (u / 2), and the comparison squares
      the returned sigma = sqrtf(q) (u): three more u than the mean's bound, on terms bounded by
      w_j 4 A^2:                                |q - ref| <= (K + 11) u 4 A^2 + ((K + 8) u A)^2
"""
import numpy as np
import pytest

import golden_replay as G
import plan_noise_ref as PN
import test_evaluate_plans_gpu as EP
from window_ref import DT

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
# (K, G, N, T): every K across a wave and a 256-thread block; G, N and T at both values
SHAPES = [(1, 1, 1, 1), (2, 3, 12, 5), (5, 3, 1, 5), (64, 1, 12, 1), (65, 3, 1, 5), (257, 1, 12, 5), (257, 3, 1, 1)]


@pytest.fixture(scope="module")
def handles(mev):
    hs = {N: EP._handle(mev, 2, N, 16, use_team=False, max_steps=0)[0] for N in (1, 12)}
    yield hs
    for h in hs.values():
        h.close()


def draw(K, Gn, N, T, seed=0):
    rng = np.random.default_rng([seed, K, Gn, N, T])
    a = rng.uniform(-1, 1, (T, Gn * K, N, 2)).astype(np.float32)
    sc = rng.normal(0, 3, Gn * K).astype(np.float32)
    return a, sc


def check_exact(tag, got, want):
    assert set(got) == set(want), tag
    for k in want:
        assert G.bits_equal(got[k], want[k]), f"{tag}: {k}"


def check_softmax(tag, got, a, scores, K, inv_t):
    x, best, top = PN.softmax_x(scores, K, inv_t)
    ref = PN.softmax64(a, x, K)
    assert np.array_equal(got["best"], best) and G.bits_equal(got["best_score"], top), tag
    w = got["weights"].astype(np.float64)
    err_w = np.abs(w - ref["weights"]) / ref["weights"].clip(1e-300)
    A = ref["A"]
    err_m = np.abs(got["new_mean"].astype(np.float64) - ref["mean"])
    q = got["new_sigma"].astype(np.float64) ** 2
    err_q = np.abs(q - ref["q"])
    bound_m = (K + 8) * U * A
    bound_q = (K + 11) * U * 4 * A * A + bound_m ** 2
    print(tag, "weights", err_w.max() / ((K + 8) * U), "mean", (err_m / bound_m).max(), "q", (err_q / bound_q).max(),
          "(fractions of the bounds)")
    assert (np.abs(w - ref["weights"]) <= (K + 8) * U * ref["weights"]).all(), tag + ": weights"
    assert (err_m <= bound_m).all(), tag + ": mean"
    assert (err_q <= bound_q).all(), tag + ": q"


@pytest.mark.parametrize("K,Gn,N,T", SHAPES)
def test_shapes(handles, K, Gn, N, T):
    h = handles[N]
    a, sc = draw(K, Gn, N, T)
    for M in sorted({1, (K + 1) // 2, K}):
        got = h.update_plans(a, K, scores=sc, mode="elites", elites=M)
        assert got["order"].shape == (Gn, M)
        check_exact(f"elites M {M}", got, PN.elites(a, sc, K, M))
    for temp in (1.0, 0.25):
        got = h.update_plans(a, K, scores=sc, mode="softmax", temperature=temp)
        assert set(got) == {"new_mean", "new_sigma", "best", "best_score", "weights"}
        check_softmax(f"softmax temperature {temp}", got, a, sc, K, np.float32(1.0 / temp))


def test_ties(handles):
    """Equal scores rank by the lower j: some equal, all equal, and -0.0 against +0.0."""
    K, Gn, N, T = 9, 3, 1, 2
    a, _ = draw(K, Gn, N, T, seed=1)
    sc = np.array([1, 3, 3, -2, 3, 1, 1, -2, 0] + [5] * K + [0.0, -0.0, -0.0, 0.0, -1, 0.0, -0.0, 2, 2], np.float32)
    got = handles[N].update_plans(a, K, scores=sc, mode="elites", elites=K)
    assert got["order"].tolist() == [[1, 2, 4, 0, 5, 6, 8, 3, 7], list(range(9, 18)), [25, 26, 18, 19, 20, 21, 23, 24, 22]]
    assert got["best"].tolist() == [1, 9, 25]
    check_exact("ties", got, PN.elites(a, sc, K, K))
    got = handles[N].update_plans(a, K, scores=sc, mode="softmax", temperature=2.0)
    assert got["best"].tolist() == [1, 9, 25]
    check_softmax("ties", got, a, sc, K, np.float32(0.5))


def test_scores_from_returns(handles):
    K, Gn, N, T = 5, 3, 12, 2
    a, _ = draw(K, Gn, N, T, seed=2)
    ret = np.random.default_rng(3).normal(0, 100, (Gn * K, N)).astype(np.float32)
    sc = PN.scores_of(ret)
    assert not G.bits_equal(sc, ret.astype(np.float64).sum(1).astype(np.float32))  # (the order of the f32 sum matters)
    h = handles[N]
    for kw in (dict(mode="elites", elites=2), dict(mode="softmax", temperature=50.0)):
        x, y = h.update_plans(a, K, returns=ret, **kw), h.update_plans(a, K, scores=sc, **kw)
        check_exact("returns " + kw["mode"], x, y)
    check_exact("returns", h.update_plans(a, K, returns=ret, mode="elites", elites=2), PN.elites(a, sc, K, 2))


def test_non_finite_scores(mev, handles):
    import torch
    torch.cuda.set_device(0)
    K, Gn, N, T = 6, 2, 1, 2
    h = handles[N]
    a, sc = draw(K, Gn, N, T, seed=4)
    sc[1], sc[4], sc[8] = np.nan, np.inf, -np.inf
    for kw in (dict(mode="elites", elites=K), dict(mode="softmax")):
        with pytest.raises(mev.MevError):
            h.update_plans(a, K, scores=sc, **kw)
    dev = "cuda:0"
    ta, ts = torch.as_tensor(a).to(dev), torch.as_tensor(sc).to(dev)
    o = dict(new_mean=torch.empty((T, Gn, N, 2), device=dev), new_sigma=torch.empty((T, Gn, N, 2), device=dev),
             best=torch.empty(Gn, dtype=torch.int32, device=dev), best_score=torch.empty(Gn, device=dev),
             order=torch.empty((Gn, K), dtype=torch.int32, device=dev))
    h.update_plans(ta, K, scores=ts, mode="elites", elites=K, out=o, device=True)
    h.sync()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    assert got["order"][0, -2:].tolist() == [1, 4] and got["order"][1, -1] == 8  # (they rank last, by j)
    check_exact("non-finite", got, PN.elites(a, sc, K, K))
    # a NaN in returns: the sum is not finite
    ret = np.ones((Gn * K, N), np.float32)
    ret[3, 0] = np.nan
    with pytest.raises(mev.MevError):
        h.update_plans(a, K, returns=ret, mode="elites", elites=1)


def test_equal_weights_and_sigma_min(handles):
    K, Gn, N, T = 65, 3, 1, 5
    h = handles[N]
    a, sc = draw(K, Gn, N, T, seed=5)
    got = h.update_plans(a, K, scores=sc, mode="softmax", temperature=float("inf"))
    assert (np.abs(got["weights"].astype(np.float64) - 1.0 / K) <= (K + 8) * U / K).all()
    check_softmax("inv_temperature 0", got, a, sc, K, np.float32(0.0))
    # sigma_min: new_sigma = fmaxf(sigma, sigma_min), the mean as without
    for kw in (dict(mode="elites", elites=7), dict(mode="softmax", temperature=1.0)):
        free = h.update_plans(a, K, scores=sc, **kw)
        floor = np.float32(np.median(free["new_sigma"]))
        held = h.update_plans(a, K, scores=sc, sigma_min=float(floor), **kw)
        assert (free["new_sigma"] < floor).any() and (free["new_sigma"] > floor).any()
        assert G.bits_equal(held["new_sigma"], np.maximum(free["new_sigma"], floor))
        assert G.bits_equal(held["new_mean"], free["new_mean"])


def test_outputs_left_null_and_errors(mev, handles):
    import torch
    torch.cuda.set_device(0)
    K, Gn, N, T = 5, 3, 12, 2
    h = handles[N]
    a, sc = draw(K, Gn, N, T, seed=6)
    dev = "cuda:0"
    ta, ts = torch.as_tensor(a).to(dev), torch.as_tensor(sc).to(dev)

    def garbage():
        shapes = dict(new_mean=((T, Gn, N, 2), torch.float32), new_sigma=((T, Gn, N, 2), torch.float32),
                      best=((Gn,), torch.int32), best_score=((Gn,), torch.float32), order=((Gn, 2), torch.int32),
                      weights=((Gn * K,), torch.float32))
        return {k: torch.full(s, 77, dtype=d, device=dev) for k, (s, d) in shapes.items()}

    want = PN.elites(a, sc, K, 2)
    for keep in (("new_mean",), ("best", "order"), ("new_sigma", "best_score")):
        o = garbage()
        h.update_plans(ta, K, scores=ts, mode="elites", elites=2, out={k: o[k] for k in keep}, device=True)
        h.sync()
        for k in o:
            if k in keep:
                assert G.bits_equal(o[k].cpu().numpy(), want[k]), k
            else:
                assert (o[k] == 77).all(), k
    # the inputs are only read
    assert G.bits_equal(ta.cpu().numpy(), a) and G.bits_equal(ts.cpu().numpy(), sc)
    ok = dict(scores=sc, mode="elites", elites=2)
    h.update_plans(a, K, **ok)
    for kw in (dict(elites=0), dict(elites=K + 1), dict(flags=mev._capi.MEV_AUTO_RESET), dict(out=dict(best=None)),
               dict(mode="softmax", temperature=-1.0), dict(mode="softmax", temperature=0.0), dict(scores=None),
               dict(sigma_min=float("nan"))):
        with pytest.raises(mev.MevError):
            h.update_plans(a, K, **dict(ok, **kw))
    big = mev._capi.MEV_MAX_SAMPLES + 1
    with pytest.raises(mev.MevError):
        h.update_plans(np.zeros((1, big, N, 2), np.float32), big, scores=np.zeros(big, np.float32), elites=1)
    with pytest.raises(mev.MevError):
        h.update_plans(np.zeros((mev._capi.MEV_MAX_REPEAT + 1, K, N, 2), np.float32), K, scores=sc[:K], elites=1)
    with pytest.raises(ValueError):
        h.update_plans(a, K, scores=sc[:-1], elites=1)
    with pytest.raises(ValueError):
        h.update_plans(a, 4, scores=sc, elites=1)


def test_largest_group(handles):
    """MEV_MAX_SAMPLES candidates in one group: the whole LDS carve."""
    K, Gn, N, T = 4096, 1, 1, 1
    a, sc = draw(K, Gn, N, T, seed=7)
    h = handles[N]
    check_exact("K 4096", h.update_plans(a, K, scores=sc, mode="elites", elites=100), PN.elites(a, sc, K, 100))
    check_softmax("K 4096", h.update_plans(a, K, scores=sc, mode="softmax", temperature=3.0), a, sc, K, np.float32(1 / 3.0))


def test_end_to_end(mev):
    """sample_plans -> update_plans(returns) -> sample_plans with the new mean and sigma."""
    E, N, T, K = 4, 2, 3, 6
    h, _ = EP._handle(mev, E, N, 16, use_team=True, max_steps=2000)
    EP._device_history_plain(h, 35, steps=6, reset_at={})
    roots = np.array([1, 3], np.int32)
    rng = np.random.default_rng(8)
    mean = rng.uniform(-0.3, 0.7, (T, 2, N, 2)).astype(np.float32)
    sigma = np.full((T, 2, N, 2), 0.5, np.float32)
    kw = dict(dt=DT, gamma=0.95, lo=(-1, -1), hi=(1, 1), seed=99)
    first = h.sample_plans(mean, sigma, roots, K, counter=0, **kw)
    assert len({first["returns"][c].tobytes() for c in range(2 * K)}) > 2  # (the candidates' returns differ)
    new = h.update_plans(first["actions_out"], K, returns=first["returns"], mode="elites", elites=2, sigma_min=0.05)
    check_exact("update", new, PN.elites(first["actions_out"], PN.scores_of(first["returns"]), K, 2, 0.05))
    second = h.sample_plans(new["new_mean"], new["new_sigma"], roots, K, counter=1, **kw)
    assert G.bits_equal(second["actions_out"],
                        PN.sampled_actions(new["new_mean"], new["new_sigma"], K, (-1, -1), (1, 1), 99, 1))
    ref = h.evaluate_plans(second["actions_out"], np.repeat(roots, K).astype(np.int32), DT, 0.95)
    for k in EP.ALL:
        assert G.bits_equal(second[k], ref[k]), k
    h.close()
