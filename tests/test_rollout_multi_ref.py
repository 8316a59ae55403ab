"""rollout_multi_ref.policy_multi_ref -- the per-slot selection among several policies that the mev_rollout_policies
tests' reference is built on -- in pure numpy, no handle: on random rows [3][11][47] the selection with one policy is
policy_ref, with identical nets it is policy_ref, relabelling the policies and `assign` consistently changes nothing,
and the noise word does not depend on the policy."""
import numpy as np

import golden_replay as G
import plan_noise_ref as PN
import policy_ref as PR
import rollout_multi_ref as RM

E, N, D = 3, 11, 47
KW = dict(lo=(-0.5, -0.25), hi=(0.75, 0.5), seed=0xABCDEF12345, counter=(7 << 32) | 5)


def net(hidden, seed):
    rng = np.random.default_rng(seed)
    dims = (D,) + tuple(hidden) + (2,)
    W = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    B = [(0.1 * rng.standard_normal(o)).astype(np.float32) for o in dims[1:]]
    return W, B


def rows(seed=1):
    return np.random.default_rng(seed).standard_normal((E, N, D)).astype(np.float32)


def same(got, want):
    assert G.bits_equal(got[0], want[0]) and G.bits_equal(got[1], want[1])


def test_one_policy_is_policy_ref():
    obs, nt = rows(), net((16, 16), 2)
    for sigma in (None, (0.3, 0.25)):
        want = PR.policy_ref(nt[0], nt[1], obs, 4, sigma, **KW)
        got = RM.policy_multi_ref([nt], np.zeros((E, N), np.uint8), obs, 4, None if sigma is None else [sigma], **KW)
        same(got, want)
        assert len(got[2]) == 1 and all(G.bits_equal(a, b) for a, b in zip(got[2][0], want[2]))


def test_identical_nets_are_policy_ref():
    obs, nt = rows(), net((16,), 3)
    assign = np.random.default_rng(4).integers(0, 4, (E, N)).astype(np.uint8)
    assert set(assign.reshape(-1)) == {0, 1, 2, 3}
    want = PR.policy_ref(nt[0], nt[1], obs, 2, (0.3, 0.25), **KW)
    same(RM.policy_multi_ref([nt] * 4, assign, obs, 2, [(0.3, 0.25)] * 4, **KW), want)


def test_relabelling_changes_nothing():
    obs = rows()
    nets = [net((16, 16), 5), net((24,), 6), net((5, 3), 7)]
    sigma = np.array([(0.3, 0.25), (0.0, 0.0), (0.1, 0.6)], np.float32)
    assign = np.random.default_rng(8).integers(0, 3, (E, N)).astype(np.uint8)
    assert set(assign.reshape(-1)) == {0, 1, 2}
    want = RM.policy_multi_ref(nets, assign, obs, 3, sigma, **KW)
    perm = np.array([2, 0, 1])  # new index q holds old policy perm[q]
    inv = np.argsort(perm).astype(np.uint8)
    got = RM.policy_multi_ref([nets[p] for p in perm], inv[assign], obs, 3, sigma[perm], **KW)
    same(got, want)
    # and the selection does select: slots of different policies differ from any single policy's rows
    for p, nt in enumerate(nets):
        one = PR.policy_ref(nt[0], nt[1], obs, 3, sigma[p], **KW)
        assert G.bits_equal(want[1][assign == p], one[1][assign == p])
        assert not G.bits_equal(want[1][assign != p], one[1][assign != p])


def test_noise_word_does_not_depend_on_the_policy():
    """With mu forced to zero (zero weights and biases) and one sigma row for all, the actions are sigma * eps of
    (e, i, t) whatever `assign` says; and straight from plan_noise_ref."""
    obs = rows()
    zero = lambda hidden: tuple([np.zeros_like(x) for x in part] for part in net(hidden, 9))
    nets = [zero((16, 16)), zero((8,)), zero((5, 3))]
    sigma = [(0.5, 0.25)] * 3
    kw = dict(KW, lo=(-9.0, -9.0), hi=(9.0, 9.0))
    rng = np.random.default_rng(10)
    a1 = RM.policy_multi_ref(nets, rng.integers(0, 3, (E, N)).astype(np.uint8), obs, 6, sigma, **kw)[0]
    a2 = RM.policy_multi_ref(nets, rng.integers(0, 3, (E, N)).astype(np.uint8), obs, 6, sigma, **kw)[0]
    e, i = np.meshgrid(np.arange(E), np.arange(N), indexing="ij")
    eps = PN.noise(kw["seed"], kw["counter"], e, i, 6)
    want = PR.act(np.zeros((E, N, 2), np.float32), sigma[0], kw["lo"], kw["hi"], eps)
    assert G.bits_equal(a1, a2) and G.bits_equal(a1, want) and len(np.unique(a1)) > E * N
