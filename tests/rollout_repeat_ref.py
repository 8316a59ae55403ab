"""numpy restatement of the loop include/marlenv.h defines mev_rollout_policy_repeat as: per decision t the
policy of policy_ref on the observation the previous decision left (noise word index t, the DECISION), then
the unchanged Handle.step_repeat with that action held for n sub-steps and spawn_route rows [t][0..n), and,
with a value head, actor_critic_ref's value chain on the hidden activations of that loop plus one more
forward pass for row T.

form="sequence" runs the same loop around Handle.step_sequence with the action row tiled n times, which the
header states equals step_repeat on every shared output; it also yields each sub-step's own done / status
rows (`sub_done`, `sub_status` [T][n][E][N], zero after the env stopped), which the tests' conditions need.

Every comparison against these results is array_equal on bits over every element (assert_all)."""
import numpy as np

import actor_critic_ref as AC
import golden_replay as G
import policy_ref as PR

SEQS = ("obs_seq", "actions_seq", "mean_seq", "reward_seq", "done_seq", "status_seq", "terminated_seq", "truncated_seq")
ALL = SEQS + ("substeps_seq",)
ALL_VALUES = ALL + ("value_seq",)


def rollout_repeat_ref(handle, weights, biases, T, n, dt=1.0 / 60.0, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0,
                       counter=0, auto_reset=False, spawn_route=None, wv=None, bv=None, form="repeat", word=None):
    """The defining loop on `handle` (which it steps).  word: the noise word index of decision t (default: t
    itself, the contract; the indexing guard passes another)."""
    E, N, D = handle.E, handle.N, handle.D
    word = (lambda t: t) if word is None else word
    seq = dict(obs_seq=np.zeros((T, E, N, D), np.float32), actions_seq=np.zeros((T, E, N, 2), np.float32),
               mean_seq=np.zeros((T, E, N, 2), np.float32), reward_seq=np.zeros((T, E, N), np.float32),
               done_seq=np.zeros((T, E, N), np.uint8), status_seq=np.zeros((T, E, N), np.uint8),
               terminated_seq=np.zeros((T, E), np.uint8), truncated_seq=np.zeros((T, E), np.uint8),
               substeps_seq=np.zeros((T, E), np.int32))
    hidden = [np.zeros((T, E, N, np.shape(W)[0]), np.float32) for W in weights[:-1]]
    npc_count = np.zeros((T, E), np.int32)
    reset_first = np.zeros((T, E), bool)  # the decision began with an auto-reset
    sub_done, sub_status = np.zeros((T, n, E, N), np.uint8), np.zeros((T, n, E, N), np.uint8)
    last = handle.get_outputs()
    ended = (last["terminated"] != 0) | (last["truncated"] != 0)
    seq["ended_before"] = ended.astype(np.uint8)
    obs = last["obs"]
    for t in range(T):
        a, mu, hid = PR.policy_ref(weights, biases, obs, word(t), sigma, lo, hi, seed, counter)
        sp = None if spawn_route is None else np.asarray(spawn_route)[t]
        reset_first[t] = ended & bool(auto_reset)
        if form == "repeat":
            r = handle.step_repeat(a, n, dt, spawn_route=sp, auto_reset=auto_reset)
        else:
            r = handle.step_sequence(np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape)), dt, spawn_route=sp,
                                     auto_reset=auto_reset)
            sub_done[t], sub_status[t] = r["done_seq"], r["status_seq"]
        obs = r["obs"].copy()
        seq["obs_seq"][t], seq["actions_seq"][t], seq["mean_seq"][t] = obs, a, mu
        seq["reward_seq"][t], seq["done_seq"][t], seq["status_seq"][t] = r["reward"], r["done"], r["status"]
        seq["terminated_seq"][t], seq["truncated_seq"][t] = r["terminated"], r["truncated"]
        seq["substeps_seq"][t] = r["substeps"]
        ended = (r["terminated"] != 0) | (r["truncated"] != 0)
        for l, x in enumerate(hid):
            hidden[l][t] = x
        npc_count[t] = handle.get_state()["npc_count"]
    seq.update(hidden=hidden, npc_count=npc_count, reset_first=reset_first, sub_done=sub_done, sub_status=sub_status)
    if wv is not None:
        seq["value_seq"] = AC.values_ref(weights, biases, wv, bv, seq)
    return seq


def assert_all(tag, out, ref, keys):
    """Every element of every named output, on bits; nothing is masked."""
    for k in keys:
        got = out[k].cpu().numpy() if hasattr(out[k], "cpu") else out[k]
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, f"{tag}: {k} shape / dtype"
        assert G.bits_equal(got, ref[k]), f"{tag}: {k}"
