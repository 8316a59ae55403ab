"""The activations of the rollout policies, without a GPU: policy_act_ref's numpy restatement of tanh_c is pinned to
mev_tanh (the host export that runs csrc/mev_act.h) bit for bit; vec_env.make_policy's parsing of every accepted and
refused module shape; and the reference's mu against the module's own float64 forward, which catches an activation
wired to the wrong layer."""
import numpy as np
import pytest

import policy_act_ref as PA

F = np.float32


def test_restatement_matches_mev_tanh(mev):
    x = PA.sweep_inputs()
    got, ref = mev._capi.tanh_c(x), PA.tanh_c(x)
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(ref[i]).hex()) for i in bad[:4]]
    assert x.size > 100000
    # the stated properties on the export itself
    pos = x[: x.size // 2]
    assert np.isnan(pos).any() and (mev._capi.tanh_c(x[np.isnan(x)]).view(np.uint32) == 0).all()  # NaN gives +0.0f
    pos = pos[~np.isnan(pos)]
    assert np.array_equal(mev._capi.tanh_c(-pos).view(np.uint32), mev._capi.tanh_c(pos).view(np.uint32) ^ np.uint32(1 << 31))
    assert (np.abs(got) <= 1).all()
    sp = mev._capi.tanh_c(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45, 10.0], F))
    assert sp.view(np.uint32).tolist() == [0, 0x80000000, 0, 0x3F800000, 0xBF800000, 0x3F800000, 0xBF800000, 1, 0x3F800000]
    assert mev._capi.tanh_c(np.zeros((2, 3), F)).shape == (2, 3)


def test_mev_tanh_refuses_bad_arguments(mev):
    import ctypes
    lib = mev.load_library()
    one = (ctypes.c_float * 1)(0.5)
    assert lib.mev_tanh(one, one, -1) == -1
    assert lib.mev_tanh(None, one, 1) == -1
    assert lib.mev_tanh(None, None, 0) == 0
    assert lib.mev_tanh(one, one, 1) == 0  # in place
    assert F(one[0]) == mev._capi.tanh_c(np.array([0.5], F))[0]


def test_make_policy_parsing(mev):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    V = mev.vec_env.VecIntersectionEnv
    L = lambda i, o, bias=True: nn.Linear(i, o, bias=bias)
    accepted = {
        ("relu", "linear"): [(L(9, 4), nn.ReLU(), L(4, 2)), (L(9, 4), nn.ReLU(), L(4, 3), nn.ReLU(), L(3, 2))],
        ("tanh", "linear"): [(L(9, 4), nn.Tanh(), L(4, 3), nn.Tanh(), L(3, 2))],
        ("relu", "tanh"): [(L(9, 4), nn.ReLU(), L(4, 2), nn.Tanh()), (L(9, 4), nn.ReLU(), L(4, 3), nn.ReLU(), L(3, 2), nn.Tanh())],
        ("tanh", "tanh"): [(L(9, 4), nn.Tanh(), L(4, 2), nn.Tanh()), (L(9, 4), nn.Tanh(), L(4, 3), nn.Tanh(), L(3, 2), nn.Tanh())],
    }
    for want, mods in accepted.items():
        for layers in mods:
            m = nn.Sequential(*layers)
            assert V._policy_activations(m) == want, (want, m)
            w, b = V._policy_arrays(m)
            lin = [x for x in layers if isinstance(x, nn.Linear)]
            assert all(a is x.weight for a, x in zip(w, lin)) and all(a is x.bias for a, x in zip(b, lin))
            assert len(w) == len(lin) == len(b)
    refused = [
        (L(9, 4), nn.Tanh(), L(4, 2)),  # (refused from a module since before tanh policies: arrays with hidden="tanh")
        (L(9, 4), nn.Sigmoid(), L(4, 2)),
        (L(9, 4), nn.ReLU(), L(4, 2), nn.ReLU()),                         # a trailing ReLU
        (L(9, 4), nn.ReLU(), L(4, 2), nn.Tanh(), nn.Tanh()),
        (L(9, 4), nn.Tanh()),
        (L(9, 2),),
        (L(9, 4), L(4, 2), nn.Tanh()),
        (L(9, 4), nn.Tanh(), L(4, 3), nn.Tanh(), L(3, 3), nn.Tanh(), L(3, 2)),  # three hidden layers
        (L(9, 4), nn.Tanh(), L(4, 2, bias=False)),
        (nn.Tanh(), L(9, 4), nn.Tanh(), L(4, 2)),
        (L(9, 4), nn.ELU(), L(4, 2), nn.Tanh()),
    ]
    for layers in refused:
        with pytest.raises(ValueError):
            V._policy_activations(nn.Sequential(*layers))
        with pytest.raises(ValueError):
            V._policy_arrays(nn.Sequential(*layers))
    for layers in ((L(9, 4), nn.ReLU(), L(4, 3), nn.Tanh(), L(3, 2)), (L(9, 4), nn.Tanh(), L(4, 3), nn.ReLU(), L(3, 2), nn.Tanh())):
        with pytest.raises(ValueError, match="same at every hidden layer"):
            V._policy_activations(nn.Sequential(*layers))
    # arrays pass through; the keywords are checked by Handle.policy's helper
    w, b = V._policy_arrays(([1, 2], [3, 4]))
    assert (w, b) == ([1, 2], [3, 4])
    C = mev._capi
    assert C.activation_flags() == 0 and C.activation_flags("tanh") == 0x10 == C.MEV_POLICY_HIDDEN_TANH
    assert C.activation_flags(out="tanh") == 0x20 == C.MEV_POLICY_OUT_TANH and C.activation_flags("tanh", "tanh") == 0x30
    for bad in (dict(hidden="gelu"), dict(out="relu"), dict(hidden=None)):
        with pytest.raises(ValueError):
            C.activation_flags(**bad)


@pytest.mark.parametrize("hidden,out,depth", [("tanh", "linear", 2), ("tanh", "tanh", 2), ("relu", "tanh", 1), ("tanh", "tanh", 1)])
def test_reference_agrees_with_the_module(hidden, out, depth):
    """policy_act_ref.forward's mu against the nn.Sequential's own forward in float64 on random rows.  A tanh on the
    wrong layer, or a missing one, moves mu by order 0.1; rounding moves it by order 1e-7.  The tolerance is 64 x the
    deviation the ReLU twin (same weights, same rows, ReLU hidden layers and a raw mu) shows against ITS float64
    forward.  Measured here: the twins deviate by 5.34e-7 (two hidden layers; tolerance 3.42e-5) and 2.61e-7 (one;
    1.67e-5), the networks under test by 2.90e-7, 2.88e-7, 2.07e-7 and 2.01e-7 in the order of the cases."""
    torch = pytest.importorskip("torch")
    nn = torch.nn
    rng = np.random.default_rng(21)
    D, widths = 40, (16, 12)[:depth]
    dims = (D,) + widths + (2,)
    W = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(F) for i, o in zip(dims[:-1], dims[1:])]
    B = [(0.3 * rng.standard_normal(o)).astype(F) for o in dims[1:]]
    x = rng.standard_normal((64, D)).astype(F)

    def module(hid, o):
        layers = []
        for l, (w, b) in enumerate(zip(W, B)):
            lin = nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
            layers.append(lin)
            if l < len(W) - 1:
                layers.append(nn.Tanh() if hid == "tanh" else nn.ReLU())
        if o == "tanh":
            layers.append(nn.Tanh())
        return nn.Sequential(*layers).double()

    def deviation(hid, o):
        net = dict(weights=W, biases=B, hidden=hid, out=o)
        with torch.no_grad():
            want = module(hid, o)(torch.from_numpy(x).double()).numpy()
        assert np.abs(want - PA.forward64(net, x)).max() < 1e-12  # (the numpy float64 forward is the module's)
        return float(np.abs(PA.forward(net, x)[0].astype(np.float64) - want).max())

    twin, got = deviation("relu", "linear"), deviation(hidden, out)
    print(f"{hidden}/{out}/{depth}: ReLU twin deviates by {twin:.3g}, this network by {got:.3g}, tolerance {64 * twin:.3g}")
    assert 0 < twin < 1e-5
    assert got <= 64 * twin
    # and the check has teeth: the twin's own mu is far outside the tolerance of this network's module
    far = np.abs(PA.forward(dict(weights=W, biases=B), x)[0] - PA.forward64(dict(weights=W, biases=B, hidden=hidden, out=out), x)).max()
    assert far > 1000 * 64 * twin
