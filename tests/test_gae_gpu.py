"""mev_gae (include/marlenv.h) against actor_critic_ref.gae_ref, bit for bit: the header's recurrence in f32,
multiply then add.  test_gae_ref.py pins gae_ref to the host build of csrc/mev_gae.h's gae_step, the text
k_gae compiles.  All inputs are finite.

The last case chains both references: Handle.rollout_policy with value_seq, then Handle.gae, on a handle
whose episodes end inside the window, against rollout_values_ref followed by gae_ref."""
import numpy as np
import pytest

import actor_critic_ref as AC
import golden_replay as G
import test_rollout_policy_gpu as RP
import test_rollout_values_gpu as RV

pytestmark = pytest.mark.gpu

SHAPES = {"5x3": (5, 3), "3x8": (3, 8), "130x1": (130, 1)}  # E N = 15: no multiple of 64; 130: more than two waves
HORIZONS = (1, 7, 33)  # 33 crosses k_gae's load batches
OUT3 = ("advantages", "returns", "valid")


def inputs(E, N, T, seed):
    rng = np.random.default_rng(seed)
    x = dict(reward=rng.uniform(-2, 2, (T, E, N)).astype(np.float32), value=rng.uniform(-30, 30, (T + 1, E, N)).astype(np.float32),
             done=(rng.random((T, E, N)) < 0.2).astype(np.uint8), terminated=(rng.random((T, E)) < 0.15).astype(np.uint8),
             truncated=(rng.random((T, E)) < 0.25).astype(np.uint8), ended_before=(rng.random(E) < 0.5).astype(np.uint8))
    # done and truncated on the same row, and ends on the last row
    x["done"][T // 2, 0, 0], x["truncated"][T // 2, 0] = 1, 1
    x["terminated"][T - 1, 1], x["truncated"][T - 1, 2], x["done"][T - 1, 0, N - 1] = 1, 1, 1
    x["ended_before"][0], x["ended_before"][1] = 1, 0
    return x


# (name, the optional arrays given, mask, outputs asked for)
OPTIONS = (
    ("bare", (), False, ("advantages", "returns")),
    ("all, masked", ("done", "terminated", "truncated", "ended_before"), True, OUT3),
    ("done + truncated, masked without ended_before", ("done", "truncated"), True, ("advantages", "valid")),
    ("terminated only", ("terminated",), False, ("returns",)),
    ("truncated + ended_before, masked", ("truncated", "ended_before"), True, ("valid", "returns")),
    ("all, unmasked", ("done", "terminated", "truncated", "ended_before"), False, OUT3),
)


def check(tag, got, x, given, mask, outputs, gamma, lam):
    kw = {k: x[k] for k in given}
    adv, ret, valid = AC.gae_ref(x["reward"], x["value"], gamma=gamma, lam=lam, mask_reset_steps=mask, **kw)
    ref = dict(advantages=adv, returns=ret, valid=valid)
    assert set(got) == set(outputs), tag
    RP.assert_seqs(tag, got, ref, outputs)
    return ref


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gae_host_pointers(mev, shape, T):
    E, N = SHAPES[shape]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=8, device=0)
    x = inputs(E, N, T, 100 + T + E)
    masked_rows = 0
    for gamma in (0.99, 1.0):
        for lam in (0.0, 0.95, 1.0):
            for name, given, mask, outputs in OPTIONS:
                kw = {k + "_seq" if k in ("done", "terminated", "truncated") else k: x[k] for k in given}
                got = h.gae(x["reward"], x["value"], gamma=gamma, lam=lam, mask_reset_steps=mask, outputs=outputs, **kw)
                ref = check(f"{shape} T={T} gamma={gamma} lam={lam} {name}", got, x, given, mask, outputs, gamma, lam)
                assert np.isfinite(ref["advantages"]).all()
                if mask:
                    masked_rows += int((ref["valid"] == 0).sum())
                else:
                    assert (ref["valid"] == 1).all()
    assert masked_rows > 0
    h.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gae_device_pointers(mev, shape):
    import torch
    torch.cuda.set_device(0)
    E, N = SHAPES[shape]
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=8, device=0)
    for T in HORIZONS:
        x = inputs(E, N, T, 200 + T + E)
        d = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
        for name, given, mask, outputs in OPTIONS[1:4]:
            kw = {k + "_seq" if k in ("done", "terminated", "truncated") else k: d[k] for k in given}
            got = h.gae(d["reward"], d["value"], gamma=0.99, lam=0.95, mask_reset_steps=mask, outputs=outputs, device=True, **kw)
            h.sync()
            assert all(v.is_cuda for v in got.values())
            check(f"{shape} T={T} device {name}", got, x, given, mask, outputs, 0.99, 0.95)
        # preallocated outputs: only those given are written
        out = dict(returns=torch.full((T, E, N), 7.0, device="cuda"))
        got = h.gae(d["reward"], d["value"], d["done"], d["terminated"], d["truncated"], gamma=1.0, lam=1.0, out=out, device=True)
        h.sync()
        assert got["returns"] is out["returns"]
        check(f"{shape} T={T} device, preallocated", got, x, ("done", "terminated", "truncated"), False, ("returns",), 1.0, 1.0)
    h.close()


def test_gae_errors(mev):
    cap = mev._capi
    E, N, T = 3, 2, 4
    h = mev.Handle(num_envs=E, num_agents=N, lidar_rays=8, device=0)
    x = inputs(E, N, T, 7)
    r, v = x["reward"], x["value"]
    with pytest.raises(mev.MevError):
        h.gae(r, v, gamma=np.nan)
    with pytest.raises(mev.MevError):
        h.gae(r, v, lam=np.inf)
    with pytest.raises(mev.MevError):
        h.gae(r, v, flags=0x2)
    with pytest.raises(mev.MevError):
        h.gae(r, v, outputs=())  # no output at all
    with pytest.raises(mev.MevError):
        h.gae(np.zeros((0, E, N), np.float32), np.zeros((1, E, N), np.float32))  # length 0
    big = cap.MEV_MAX_ROLLOUT + 1
    with pytest.raises(mev.MevError):
        h.gae(np.zeros((big, E, N), np.float32), np.zeros((big + 1, E, N), np.float32))
    import ctypes
    ga = cap.MevGaeArgs()
    ga.length, ga.gamma, ga.lam = T, 0.99, 0.95
    adv = np.zeros((T, E, N), np.float32)
    ga.advantages = cap._ptr(adv)
    lib = mev.load_library()
    assert lib.mev_gae(h._h, ctypes.byref(ga)) != 0  # null rewards and values
    ga.reward_seq = cap._ptr(r)
    assert lib.mev_gae(h._h, ctypes.byref(ga)) != 0  # null values
    with pytest.raises(ValueError):
        h.gae(r, v[:-1])
    got = h.gae(r, v)  # and the handle still serves the call
    check("after the refused calls", got, x, (), False, ("advantages", "returns"), 0.99, 0.95)
    h.close()


# ---- end to end: rollout with values, then gae, both references chained ----

def test_rollout_then_gae(mev):
    E, N, rays, T = 5, 3, 16, 7
    mk = lambda: RP.make(mev, E, N, rays, history=1, max_steps=3, respawn=True)
    A, B = mk(), mk()
    W, Bs = RP.net(127, (16, 16), 51, steer=0.9)
    wv, bv = RV.head(16, 52)
    pol = A.policy(W, Bs)
    pol.set_value_head(wv, bv)
    kw = dict(dt=1.0, auto_reset=True)
    for window in range(2):  # the second window's ended_before comes from the first's last row
        last = A.get_outputs()
        eb = ((last["terminated"] != 0) | (last["truncated"] != 0)).astype(np.uint8)
        out = A.rollout_policy(pol, T, outputs=RV.WITH_VALUES, **kw)
        ref = AC.rollout_values_ref(B, W, Bs, wv, bv, T, **kw)
        RP.assert_seqs(f"window {window}", out, ref, RV.WITH_VALUES)
        assert G.bits_equal(eb, ref["ended_before"])
        got = A.gae(out["reward_seq"], out["value_seq"], out["done_seq"], out["terminated_seq"], out["truncated_seq"], eb,
                    gamma=0.99, lam=0.95, mask_reset_steps=True, outputs=OUT3)
        adv, ret, valid = AC.gae_ref(ref["reward_seq"], ref["value_seq"], ref["done_seq"], ref["terminated_seq"],
                                     ref["truncated_seq"], ref["ended_before"], 0.99, 0.95, True)
        RP.assert_seqs(f"window {window} gae", got, dict(advantages=adv, returns=ret, valid=valid), OUT3)
        ended = (ref["terminated_seq"] | ref["truncated_seq"]) != 0
        assert ended[:-1].any() and (ref["truncated_seq"] != 0).any()
        # the masked rows are exactly those that follow an env's end
        before = np.concatenate([ref["ended_before"][None] != 0, ended[:-1]])
        assert np.array_equal(valid == 0, np.broadcast_to(before[:, :, None], valid.shape))
        assert (adv[valid == 0] == 0).all()
    RP.same_handles("after rollout + gae", A, B)  # mev_gae touched nothing of the handle
    A.close(), B.close()
