"""numpy restatement of the loop include/marlenv.h defines mev_rollout_policies as: rollout_repeat_ref's loop with
one line changed -- agent slot (e, i) is driven by nets[assign[e][i]].  Per decision every listed policy's
policy_ref runs on the whole observation (its own layers and its own sigma row; the noise word is the slot's and the
decision's, whatever the policy), and the action, mean and value rows are selected per (e, i) by `assign`, which
holds for the whole call.  The step is the unchanged Handle.step_repeat; the value rows are actor_critic_ref's
values_ref of each policy on its own hidden activations, selected the same way.

A net is (weights, biases) or (weights, biases, wv, bv).  Every comparison against these results is on bits over
every element (rollout_repeat_ref.assert_all)."""
import numpy as np

import actor_critic_ref as AC
import policy_ref as PR


def select(assign, rows):
    """out[e][i] = rows[assign[e][i]][e][i] for per-policy arrays rows[p] of one shape [E][N]..."""
    assign = np.asarray(assign)
    out = np.array(rows[0], copy=True)
    for p in range(1, len(rows)):
        out[assign == p] = np.asarray(rows[p])[assign == p]
    return out


def policy_multi_ref(nets, assign, obs, t, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0, counter=0):
    """(actions, mu, hidden) for obs [E][N][D]: policy_ref of every listed policy -- sigma[p] its row, the noise word
    that of (e, i, t) -- selected by assign; hidden[p] is policy p's own list of activations over ALL slots."""
    per = [PR.policy_ref(net[0], net[1], obs, t, None if sigma is None else sigma[p], lo, hi, seed, counter)
           for p, net in enumerate(nets)]
    return select(assign, [r[0] for r in per]), select(assign, [r[1] for r in per]), [r[2] for r in per]


def rollout_multi_ref(handle, nets, assign, T, n, sigma=None, dt=1.0 / 60.0, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed=0,
                      counter=0, auto_reset=False, spawn_route=None):
    """The defining loop on `handle` (which it steps); the keys of rollout_repeat_ref's result -- value_seq where
    every net has a head -- plus `hidden` [p][layer] ([T][E][N][width]), `npc_count` and `reset_first`."""
    E, N, D = handle.E, handle.N, handle.D
    assign = np.asarray(assign, np.uint8)
    assert assign.shape == (E, N) and int(assign.max()) < len(nets)
    seq = dict(obs_seq=np.zeros((T, E, N, D), np.float32), actions_seq=np.zeros((T, E, N, 2), np.float32),
               mean_seq=np.zeros((T, E, N, 2), np.float32), reward_seq=np.zeros((T, E, N), np.float32),
               done_seq=np.zeros((T, E, N), np.uint8), status_seq=np.zeros((T, E, N), np.uint8),
               terminated_seq=np.zeros((T, E), np.uint8), truncated_seq=np.zeros((T, E), np.uint8),
               substeps_seq=np.zeros((T, E), np.int32))
    hidden = [[np.zeros((T, E, N, np.shape(W)[0]), np.float32) for W in net[0][:-1]] for net in nets]
    npc_count = np.zeros((T, E), np.int32)
    reset_first = np.zeros((T, E), bool)  # the decision began with an auto-reset
    last = handle.get_outputs()
    ended = (last["terminated"] != 0) | (last["truncated"] != 0)
    seq["ended_before"] = ended.astype(np.uint8)
    obs = last["obs"]
    for t in range(T):
        a, mu, hid = policy_multi_ref(nets, assign, obs, t, sigma, lo, hi, seed, counter)
        sp = None if spawn_route is None else np.asarray(spawn_route)[t]
        reset_first[t] = ended & bool(auto_reset)
        r = handle.step_repeat(a, n, dt, spawn_route=sp, auto_reset=auto_reset)
        obs = r["obs"].copy()
        seq["obs_seq"][t], seq["actions_seq"][t], seq["mean_seq"][t] = obs, a, mu
        seq["reward_seq"][t], seq["done_seq"][t], seq["status_seq"][t] = r["reward"], r["done"], r["status"]
        seq["terminated_seq"][t], seq["truncated_seq"][t] = r["terminated"], r["truncated"]
        seq["substeps_seq"][t] = r["substeps"]
        ended = (r["terminated"] != 0) | (r["truncated"] != 0)
        for p, layers in enumerate(hid):
            for l, x in enumerate(layers):
                hidden[p][l][t] = x
        npc_count[t] = handle.get_state()["npc_count"]
    seq.update(hidden=hidden, npc_count=npc_count, reset_first=reset_first)
    if all(len(net) == 4 for net in nets):
        rows = [AC.values_ref(net[0], net[1], net[2], net[3], dict(obs_seq=seq["obs_seq"], hidden=hidden[p]))
                for p, net in enumerate(nets)]
        seq["value_seq"] = select(np.broadcast_to(assign, (T + 1, E, N)), rows)
    return seq
