"""policy_ref.fma32 -- the float64 construction of an exactly rounded f32 fmaf that the rollout tests'
host policy is built on -- against libm's fmaf (through ctypes): random triples, triples forced onto f32
ties (where a double rounding would show), subnormal products, and a 39-16-16-2 layer stack."""
import numpy as np

import golden_replay as G
import policy_ref as PR


def _same(a, b, c):
    got, want = PR.fma32(a, b, c), PR.fmaf_libm(a, b, c)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (a[bad[:3]], b[bad[:3]], c[bad[:3]], got[bad[:3]], want[bad[:3]])


def test_random_triples():
    rng = np.random.default_rng(1)
    n = 40000
    a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    _same(a, b, c)
    # wide exponents, and sums that cancel to a few bits
    sc = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
    a, b = sc(), sc()
    _same(a, b, sc())
    _same(a, b, (-(a.astype(np.float64) * b) * (1 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(np.float32))


def test_forced_ties():
    """a * b + c lies exactly on the midpoint of two adjacent floats, or beside it by less than float64's
    last bit: rounding the sum to 53 bits first and then to 24 would take such a value as the tie."""
    rng = np.random.default_rng(2)
    n = 4096
    k = rng.integers(1, 2048, n)
    # the product carries the tie: (1 + k 2^-12)(1 + 2^-12) = 1 + (k + 1) 2^-12 + k 2^-24, k odd -> a midpoint
    a = (1.0 + (2 * k + 1) * 2.0 ** -12).astype(np.float32)
    b = np.full(n, np.float32(1.0 + 2.0 ** -12))
    prod = a.astype(np.float64) * b
    assert (np.ldexp(prod, 24) % 2 == 1).all()  # (an odd multiple of 2^-24 in [1, 4): not a float32)
    _same(a, b, np.zeros(n, np.float32))
    for e in (-60, -80, -100, -140):  # beside the tie by 2^e, below float64's resolution of the sum
        for sign in (1.0, -1.0):
            _same(a, b, np.full(n, np.float32(sign * 2.0 ** e)))
            _same(-a, b, np.full(n, np.float32(sign * 2.0 ** e)))
    # c carries the head and the product the half ulp, with and without a sticky part
    c = rng.uniform(1.0, 2.0, n).astype(np.float32)
    half = np.full(n, np.float32(2.0 ** -24))
    _same(half, np.ones(n, np.float32), c)
    _same(half, np.full(n, np.float32(1.0 + 2.0 ** -23)), c)
    _same(half, np.full(n, np.float32(1.0 - 2.0 ** -24)), c)
    _same(half, np.ones(n, np.float32), -c)
    # cancellation: the head cancels and the tie sits in what is left
    _same(a, b, np.full(n, np.float32(-1.0)))
    _same(a, b, (-a).astype(np.float32))


def test_subnormal_products():
    rng = np.random.default_rng(3)
    n = 20000
    a = (rng.standard_normal(n) * 1e-30).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-60, -36, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-149, -120, n))).astype(np.float32)
    prod = a.astype(np.float64) * b
    assert (np.abs(prod) < 2.0 ** -126).all() and (prod != 0).any()
    _same(a, b, c)
    _same(a, b, np.zeros(n, np.float32))
    tiny = np.float32(2.0 ** -149)
    _same(np.full(n, tiny), rng.uniform(0.25, 0.75, n).astype(np.float32), (rng.integers(0, 5, n) * tiny).astype(np.float32))


def test_layer_stack():
    """39-16-16-2: the vectorised chain equals the same chain over libm's fmaf, and the ReLU's corner cases."""
    rng = np.random.default_rng(4)
    dims = (39, 16, 16, 2)
    Ws = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [rng.standard_normal(o).astype(np.float32) * np.float32(0.1) for o in dims[1:]]
    x = rng.standard_normal((5, 3, 39)).astype(np.float32)
    mu, hid = PR.forward(Ws, bs, x)
    mu2, hid2 = PR.forward(Ws, bs, x, fma=PR.fmaf_libm)
    assert mu.shape == (5, 3, 2) and [h.shape[-1] for h in hid] == [16, 16]
    assert G.bits_equal(mu, mu2) and all(G.bits_equal(p, q) for p, q in zip(hid, hid2))
    assert all((h == 0).any() and (h > 0).any() for h in hid)
    r = PR.relu(np.array([np.nan, -0.0, -1.0, 2.0], np.float32))
    assert G.bits_equal(r, np.array([0.0, 0.0, 0.0, 2.0], np.float32))
    a = PR.act(np.array([[-3.0, 0.25]], np.float32), None, (-1.0, -0.5), (1.0, 0.5))
    assert G.bits_equal(a, np.array([[-1.0, 0.25]], np.float32))
