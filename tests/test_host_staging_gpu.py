"""Host-mode calls of many kinds sharing the handle's one staging block (csrc/mev_capi.cpp, Stage).
Two handles in the same state run one sequence of calls: A in host mode with numpy arrays, which
stages every array in the block, B with device=True and torch tensors, which never touches it.  The
sequence makes the block grow (the leaf observations of 25 candidates), then reuses it at smaller
sizes, so that one call's outputs lie where the previous call's inputs were.  Every output of every
call on A must equal B's bit for bit, and so must the handles' and the pools' states at the end.
Every output buffer is filled with 0xFF bytes before its call, on both sides."""
import numpy as np
import pytest

import golden_replay as G
import window_ref as RR
from test_evaluate_leaves_gpu import filled, outputs
from window_ref import DT, OUT_KEYS

pytestmark = pytest.mark.gpu

E, N, RAYS, NPCS = 5, 3, 16, 8
DEV = "cuda:0"


def _pair(mev):
    """Two handles, traffic on, after the same 12 host-mode steps with replayed spawns."""
    hs = []
    for _ in range(2):
        h = RR.handle(mev, E, N, RAYS, traffic=True, density=5.0, max_npcs=NPCS)
        RR.set_routes(h, True)
        rng = np.random.default_rng(11)
        for _ in range(12):
            h.step(RR.draw(rng, E, N, 1.0)[0], DT, spawn_route=rng.integers(-1, 12, E))
        hs.append(h)
    return hs


def _step_out(h, T=None):
    """The step's outputs plus substeps and, for a plan of T rows, the *_seq rows: 0xFF bytes."""
    o = {k: filled(v.shape, v.dtype) for k, v in h.alloc_outputs().items()}
    o["substeps"] = filled((E,), np.int32)
    if T is not None:
        o.update(reward_seq=filled((T, E, N), np.float32), done_seq=filled((T, E, N), np.uint8),
                 status_seq=filled((T, E, N), np.uint8))
    return o


def _same(tag, a, b):
    assert set(a) == set(b), tag
    for k in a:
        assert G.bits_equal(a[k], b[k]), f"{tag}: {k}"


def test_host_calls_share_one_block(mev):
    import torch
    torch.cuda.set_device(0)
    A, B = _pair(mev)
    _same("start", A.get_state(), B.get_state())
    rng = np.random.default_rng(5)
    held = []  # B's tensors: its last outputs live in the caller's memory

    def t(x):
        x = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
        held.append(x)
        return x

    def both(tag, call, out, **arrays):
        """call(h, out, device, **arrays) on A with numpy and on B with tensors; every output compared."""
        got = call(A, {k: v.copy() for k, v in out.items()}, False, **arrays)
        dev = {k: t(v) for k, v in out.items()}
        call(B, dev, True, **{k: t(v) for k, v in arrays.items()})
        B.sync()
        _same(tag, got, {k: v.cpu().numpy() for k, v in dev.items()})
        return got

    def plan_of(C, T, traffic=True):
        """actions [T][C][N][2], dts [T], spawn routes [T][C] (int32, as device mode takes them)"""
        a, dts, sp = RR.draw_plan(rng, C, N, T, 0.7, traffic)
        return a, dts, sp.astype(np.int32) if traffic else None

    def sequence(T):
        a, dts, sp = plan_of(E, T)
        both(f"step_sequence T = {T}", lambda h, o, d, a, sp: h.step_sequence(a, dts, o, sp, device=d),
             _step_out(A, T), a=a, sp=sp)

    def states(tag):
        _same(tag, A.get_state(), B.get_state())
        _same(tag + ": outputs", A.get_outputs(), B.get_outputs())

    sequence(2)
    # 25 candidates with leaf observations: the block grows
    T, C = 3, 5 * E
    a, dts, sp = plan_of(C, T)
    both("evaluate_plans with leaf_obs",
         lambda h, o, d, a, r, sp: h.evaluate_plans(a, r, dts, 0.95, sp, o, d, leaf_obs=True),
         outputs(T, C, N, A.D), a=a, r=rng.integers(0, E, C).astype(np.int32), sp=sp)
    # pools: a capture, then an expansion from the pool into the pool (candidate 3's stop state not kept)
    pool = {A: A.pool(3 * E), B: B.pool(3 * E)}
    envs, slots = np.arange(E, dtype=np.int32)[::-1], np.arange(E, dtype=np.int32)
    pool[A].capture(envs, slots)
    pool[B].capture(t(envs), t(slots), device=True)
    C = 2 * E
    a, dts, sp = plan_of(C, T)
    dst = (E + np.arange(C)).astype(np.int32)
    dst[3] = -1
    both("expand_plans",
         lambda h, o, d, a, r, ds, sp: h.expand_plans(a, r, pool[h], ds, pool[h], 1, True, dts, 0.9, sp, o, d),
         outputs(T, C, N, A.D), a=a, r=(np.arange(C) % E).astype(np.int32), ds=dst, sp=sp)
    # sampling, then both refits over the sampled candidates
    Gr, K = 4, 6
    C = Gr * K
    so = dict(outputs(T, C, N), actions_out=filled((T, C, N, 2), np.float32))
    drawn = both("sample_plans",
                 lambda h, o, d, m, s, r: h.sample_plans(m, s, r, K, dts, 0.9, seed=3, counter=9, out=o, device=d), so,
                 m=rng.uniform(-0.5, 0.5, (T, Gr, N, 2)).astype(np.float32),
                 s=rng.uniform(0.1, 0.5, (T, Gr, N, 2)).astype(np.float32), r=rng.integers(0, E, Gr).astype(np.int32))
    uo = dict(new_mean=filled((T, Gr, N, 2), np.float32), new_sigma=filled((T, Gr, N, 2), np.float32),
              best=filled((Gr,), np.int32), best_score=filled((Gr,), np.float32))
    both("update_plans, elites",
         lambda h, o, d, a, r: h.update_plans(a, K, returns=r, mode="elites", elites=2, sigma_min=0.05, out=o, device=d),
         dict(uo, order=filled((Gr, 2), np.int32)), a=drawn["actions_out"], r=drawn["returns"])
    both("update_plans, softmax",
         lambda h, o, d, a, s: h.update_plans(a, K, scores=s, mode="softmax", temperature=0.5, out=o, device=d),
         dict(uo, weights=filled((C,), np.float32)), a=drawn["actions_out"],
         s=drawn["returns"].sum(1, dtype=np.float32))
    # frame skip, a host snapshot (B: a device one), one more step, then the two per-env restores
    a, sp = RR.draw(rng, E, N, 0.8, 3, traffic=True)
    both("step_repeat", lambda h, o, d, a, sp: h.step_repeat(a, 3, DT, o, sp, device=d), _step_out(A),
         a=a, sp=sp.astype(np.int32))
    snap = A.snapshot()
    dsnap = t(np.zeros(B.snapshot_size(), np.uint8))
    B.snapshot(dsnap, device=True)
    assert G.bits_equal(snap, dsnap.cpu().numpy()), "snapshot bytes"
    a, sp = RR.draw(rng, E, N, 0.8, 1, traffic=True)
    both("step", lambda h, o, d, a, sp: h.step(a, DT, o, sp, device=d),
         {k: v for k, v in _step_out(A).items() if k in OUT_KEYS}, a=a, sp=sp[0].astype(np.int32))
    ahead = A.get_state()
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    A.restore(snap, env_mask=mask)
    B.restore(dsnap, env_mask=t(mask), device=True)
    B.sync()
    states("masked restore")
    now = A.get_state()  # (the masked envs went back a step, the others stayed)
    assert G.bits_equal(now["y"][mask == 0], ahead["y"][mask == 0]) and G.bits_equal(now["x"][mask == 0], ahead["x"][mask == 0])
    assert not (G.bits_equal(now["y"][mask == 1], ahead["y"][mask == 1]) and G.bits_equal(now["x"][mask == 1], ahead["x"][mask == 1]))
    env_map = np.array([3, -1, 0, 0, 1], np.int32)
    A.restore(snap, env_map=env_map)
    B.restore(dsnap, env_map=t(env_map), device=True)
    B.sync()
    states("restore_map")
    # smaller calls in the grown block
    sequence(5)
    a, dts, _ = plan_of(2, 4, traffic=False)
    both("evaluate_plans C = 2", lambda h, o, d, a, r: h.evaluate_plans(a, r, dts, 1.0, None, o, d), outputs(4, 2, N),
         a=a, r=np.array([4, 0], np.int32))
    # the states the calls left
    states("end")
    every = np.arange(3 * E)
    (sa, da, va), (sb, db, vb) = pool[A].get_state(every), pool[B].get_state(every)
    assert va.tolist() == vb.tolist() == [1] * E + [0 if c == 3 else 1 for c in range(2 * E)]
    _same("pool", sa, sb)
    assert G.bits_equal(da[0], db[0]) and G.bits_equal(da[1], db[1]), "pool: car sizes"
    A.close()
    B.close()
