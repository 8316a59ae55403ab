"""Batched environment: E independent intersections advanced by one device
call per step (BASELINE north star; the reference steps one env per Python
call, reference env.py:152-195 / cpp/IntersectionEnv.cpp:133-392).

Two modes:
 * backend="torch": actions and outputs are CUDA (HIP) tensors on `device`;
   every step is one asynchronous launch pair ordered on torch's current
   stream, no host round trip.  The returned tensors are this env's output
   buffers and are overwritten by the next step (pass copy=True to clone).
 * backend="numpy": host arrays in and out (synchronous; for tests and
   small-scale use).

Per-agent semantics are exactly the reference's (bit-exact, see tests/);
auto_reset=True restarts an env in the step after it reported terminated or
truncated, which is what an RL rollout loop does with the reference env.

max_npcs (NPC slots per env, traffic mode) defaults to 32, the C ABI's default:
spawned traffic never holds more than 15 NPCs in one env (the reference's spawn
test, profiles/r6_fleet_probe.txt), and 32 slots run the compile-time one-ego
kernel (4096 envs at density 0.5: 159 M agent-steps/s against 75 M with 64
slots, profiles/r6_cfg4_k64.txt).  Pass max_npcs=64 to write up to 64 traffic
cars per env through set_state.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _capi
from .utils import default_routes, point_index

_REWARD_ORDER = ("progress_scale", "stuck_speed_threshold", "stuck_penalty", "crash_vehicle_penalty",
                 "crash_object_penalty", "success_reward", "action_smoothness_scale", "team_alpha")
_REWARD_DEFAULT = (10.0, 1.0, -0.01, -10.0, -5.0, 10.0, -0.02, 0.2)


def reward_vector(reward_config) -> list:
    """env.py-style reward dict (or an 8-list in RewardConfig order) -> the C-ABI reward[8]."""
    if reward_config is None:
        return list(_REWARD_DEFAULT)
    if isinstance(reward_config, dict):
        return [float(reward_config.get(k, d)) for k, d in zip(_REWARD_ORDER, _REWARD_DEFAULT)]
    v = [float(x) for x in reward_config]
    if len(v) != 8:
        raise ValueError("reward_config must have 8 entries")
    return v


class VecIntersectionEnv:
    def __init__(self, num_envs: int, num_agents: int = 8, num_lanes: int = 3, lidar_rays: int = 96,
                 obs_dim: Optional[int] = None, use_team_reward: bool = False, respawn_enabled: bool = True,
                 max_steps: int = 2000, traffic_flow: bool = False, traffic_density: float = 0.5,
                 reward_config: Any = None, ego_routes: Optional[Sequence] = None, max_npcs: int = 32,
                 seed: int = 0, device: int = 0, backend: str = "torch", auto_reset: bool = True,
                 lidar_fov_deg: float = 360.0, lidar_max_dist: float = 250.0, lidar_step: float = 4.0,
                 frame_skip: int = 1):
        if not 1 <= int(frame_skip) <= _capi.MEV_MAX_REPEAT:
            raise ValueError(f"frame_skip must be in 1..{_capi.MEV_MAX_REPEAT}")
        self.frame_skip = int(frame_skip)
        if backend not in ("torch", "numpy"):
            raise ValueError("backend must be 'torch' or 'numpy'")
        if traffic_flow and num_agents != 1:
            raise ValueError("traffic_flow mode has exactly one ego per env (reference env.py:84-87)")
        self.backend = backend
        self.auto_reset = bool(auto_reset)
        self.num_envs, self.num_agents, self.num_lanes = int(num_envs), int(num_agents), int(num_lanes)
        if obs_dim is None:
            obs_dim = 127 if lidar_rays <= 96 else 31 + lidar_rays
        self._h = _capi.Handle(num_envs=self.num_envs, num_agents=self.num_agents, num_lanes=self.num_lanes,
                               lidar_rays=int(lidar_rays), lidar_fov_deg=float(lidar_fov_deg),
                               lidar_max_dist=float(lidar_max_dist), lidar_step=float(lidar_step),
                               obs_dim=int(obs_dim), traffic_flow=int(bool(traffic_flow)),
                               traffic_density=float(traffic_density), use_team_reward=int(bool(use_team_reward)),
                               respawn_enabled=int(bool(respawn_enabled)), max_steps=int(max_steps),
                               reward=reward_vector(reward_config), max_npcs=int(max_npcs), seed=int(seed),
                               device=int(device))
        self.obs_dim = self._h.D
        self.device_index = int(device)
        if ego_routes is not None:
            self.set_ego_routes(ego_routes)
        self._stream = None
        self._out = None
        if backend == "torch":
            import torch
            self._torch = torch
            dev = torch.device("cuda", self.device_index)
            E, N, D = self.num_envs, self.num_agents, self.obs_dim
            self._out = dict(obs=torch.zeros((E, N, D), dtype=torch.float32, device=dev),
                             reward=torch.zeros((E, N), dtype=torch.float32, device=dev),
                             done=torch.zeros((E, N), dtype=torch.uint8, device=dev),
                             status=torch.zeros((E, N), dtype=torch.uint8, device=dev),
                             terminated=torch.zeros(E, dtype=torch.uint8, device=dev),
                             truncated=torch.zeros(E, dtype=torch.uint8, device=dev),
                             agents_alive=torch.zeros(E, dtype=torch.int32, device=dev),
                             step=torch.zeros(E, dtype=torch.int32, device=dev))
            self._bind_stream()
        else:
            self._out = self._h.alloc_outputs()
        self._out_rep = None  # the same buffers plus `substeps`, made at the first frame-skip step
        self._out_seq = None  # ... plus the per-step rows of a plan rollout (step_sequence), per plan length
        self._out_eval = {}   # (T, C) -> the outputs of evaluate_plans

    # ----------------------------------------------------------------- utils
    @property
    def handle(self) -> _capi.Handle:
        return self._h

    def _bind_stream(self):
        s = self._torch.cuda.current_stream(self.device_index)
        if s.cuda_stream != self._stream:
            self._h.set_stream(s.cuda_stream)
            self._stream = s.cuda_stream

    def set_ego_routes(self, routes):
        """routes: [(start, end)] names per agent (same for every env), or an int array [E, N] of route ids."""
        if len(routes) and isinstance(routes[0], (tuple, list)) and isinstance(routes[0][0], str):
            P = 8 * self.num_lanes
            ids = []
            for s, e in routes:
                si, ei = point_index(s, self.num_lanes), point_index(e, self.num_lanes)
                if si < 0 or ei < 0:
                    raise IndexError(f"unknown lane id in route ({s!r}, {e!r})")
                ids.append(si * P + ei)
            routes = np.asarray(ids, np.int32)
        self._h.set_ego_routes(np.asarray(routes, np.int32))

    def set_reset_routes(self, routes):
        """Draw every agent's route from `routes` (names or ids) at each reset, as the
        reference test.py does with random.choice(all_routes); [] restores fixed routes."""
        ids = []
        P = 8 * self.num_lanes
        for r in routes:
            if isinstance(r, (tuple, list)):
                si, ei = point_index(r[0], self.num_lanes), point_index(r[1], self.num_lanes)
                if si < 0 or ei < 0:
                    raise IndexError(f"unknown lane id in route {tuple(r)!r}")
                ids.append(si * P + ei)
            else:
                ids.append(int(r))
        self._h.set_reset_routes(ids)

    def snapshot(self, out=None):
        """Whole-batch state + last outputs (torch: a device uint8 tensor; numpy: host bytes)."""
        if self.backend == "torch":
            self._bind_stream()
            if out is None:
                out = self._torch.empty(self._h.snapshot_size(), dtype=self._torch.uint8,
                                        device=self._out["obs"].device)
            self._h.snapshot(out, device=True)
            return out
        return self._h.snapshot(out)

    def restore(self, snap, env_mask=None, env_map=None):
        """Roll all envs (or those with env_mask != 0) back to `snap`; outputs follow.
        env_map ([E] ints): env e takes the state and outputs of the snapshot's env env_map[e]
        (-1 leaves it alone) -- fan one root env out into E candidates (Handle.restore)."""
        if env_mask is not None and env_map is not None:
            raise ValueError("pass env_mask or env_map, not both")
        if self.backend == "torch":
            self._bind_stream()
            mask = emap = None
            if env_mask is not None:
                mask = self._torch.as_tensor(env_mask, device=self._out["obs"].device).to(self._torch.uint8)
                mask = mask.contiguous()
            if env_map is not None:
                emap = self._torch.as_tensor(env_map, device=self._out["obs"].device).to(self._torch.int32)
                emap = emap.contiguous()
                if emap.numel() != self.num_envs:
                    raise ValueError(f"env_map must have {self.num_envs} entries, got {tuple(emap.shape)}")
            self._h.restore(snap, env_mask=mask, env_map=emap, device=True)
            self._h.get_outputs(self._out, device=True)
            return self._out["obs"]
        self._h.restore(snap, env_mask=env_mask, env_map=env_map)
        return self._h.get_outputs(self._out)["obs"]

    def set_traffic_routes(self, routes):
        """The NPC route list (reference configure_routes); names or route ids."""
        P = 8 * self.num_lanes
        ids = []
        for r in routes:
            if isinstance(r, (tuple, list)):
                si, ei = point_index(r[0], self.num_lanes), point_index(r[1], self.num_lanes)
                if si < 0 or ei < 0:
                    raise IndexError(f"unknown lane id in route {tuple(r)!r}")
                ids.append(si * P + ei)
            else:
                ids.append(int(r))
        self._h.set_traffic_routes(np.asarray(ids, np.int32))

    # ------------------------------------------------------------- episode
    def reset(self, env_mask=None):
        """Reset all envs (or those with env_mask != 0); returns the observation buffer."""
        if self.backend == "torch":
            self._bind_stream()
            mask = None
            if env_mask is not None:
                mask = self._torch.as_tensor(env_mask, device=self._out["obs"].device).to(self._torch.uint8)
                mask = mask.contiguous()
            self._h.reset(env_mask=mask, obs=self._out["obs"], device=True)
            return self._out["obs"]
        self._h.reset(env_mask=env_mask, obs=self._out["obs"])
        return self._out["obs"]

    def step(self, actions, dt: float = 1.0 / 60.0, copy: bool = False, spawn_route=None, repeat: Optional[int] = None):
        """actions [E, N, 2] (throttle, steer) -> (obs, rewards, terminated, truncated, info).
        repeat (default: the constructor's frame_skip) > 1 holds the actions for up to that many
        sub-steps in one device call (Handle.step_repeat): rewards are summed, done / status
        latched, each env stops at its first terminated or truncated sub-step, the LiDAR is cast
        once, and info["substeps"] [E] says how many sub-steps each env ran; spawn_route is then
        [repeat][E]."""
        n = self.frame_skip if repeat is None else int(repeat)
        o = self._out if n == 1 else self._window_out()
        if self.backend == "torch":
            self._bind_stream()
            a = self._actions_tensor(actions, plan=False)
            sp = self._spawn_tensor(spawn_route)
            if n == 1:
                self._h.step(a, float(dt), out=o, spawn_route=sp, auto_reset=self.auto_reset, device=True)
            else:
                self._h.step_repeat(a, n, float(dt), out=o, spawn_route=sp, auto_reset=self.auto_reset, device=True)
            if copy:
                o = {k: v.clone() for k, v in o.items()}
        else:
            if n == 1:
                self._h.step(actions, float(dt), out=o, spawn_route=spawn_route, auto_reset=self.auto_reset)
            else:
                self._h.step_repeat(actions, n, float(dt), out=o, spawn_route=spawn_route, auto_reset=self.auto_reset)
            if copy:
                o = {k: v.copy() for k, v in o.items()}
        info = {"done": o["done"], "status": o["status"], "agents_alive": o["agents_alive"], "step": o["step"]}
        if n > 1:
            info["substeps"] = o["substeps"]
        return o["obs"], o["reward"], o["terminated"], o["truncated"], info

    def step_sequence(self, actions, dt=1.0 / 60.0, spawn_route=None, copy: bool = False):
        """Open-loop plan rollout: actions [T, E, N, 2], one action row per sub-step (dt: a float or
        T host floats) -> (obs, rewards, terminated, truncated, info) in one device call
        (Handle.step_sequence).  obs is the leaf observation (one LiDAR cast), rewards the
        per-agent sums; info holds done / status / agents_alive / step as after `step`, plus
        substeps [E] and reward_seq / done_seq / status_seq [T, E, N]: each executed sub-step's own
        outputs, zero after an env stopped (terminated or truncated), so a discounted sum over
        the T rows needs no mask.  spawn_route, if given, is [T][E].  torch: stream-ordered on
        the current stream, zero-copy; the returned tensors are reused by the next call with
        the same T."""
        if self.backend == "torch":
            self._bind_stream()
            a = self._actions_tensor(actions, plan=True)
            T = int(a.shape[0])
            o = self._window_out(T)
            sp = self._spawn_tensor(spawn_route, T)
            self._h.step_sequence(a, dt, out=o, spawn_route=sp, auto_reset=self.auto_reset, device=True, length=T)
            if copy:
                o = {k: v.clone() for k, v in o.items()}
        else:
            T = int(np.shape(actions)[0])
            o = self._window_out(T)
            self._h.step_sequence(actions, dt, out=o, spawn_route=spawn_route, auto_reset=self.auto_reset)
            if copy:
                o = {k: v.copy() for k, v in o.items()}
        info = {k: o[k] for k in ("done", "status", "agents_alive", "step", "substeps", "reward_seq", "done_seq",
                                  "status_seq")}
        return o["obs"], o["reward"], o["terminated"], o["truncated"], info

    def _dev_tensor(self, x, dtype):
        """x as a contiguous tensor of `dtype` on this env's device (torch backend)."""
        t = self._torch
        if isinstance(x, t.Tensor) and x.is_cuda and x.dtype == dtype and x.is_contiguous():
            if x.device.index != self.device_index:
                raise ValueError("an argument is on another device")
            return x
        return t.as_tensor(x, dtype=dtype, device=self._out["obs"].device).contiguous()

    def evaluate_plans(self, actions, roots, dt=1.0 / 60.0, gamma: float = 1.0, spawn_route=None, copy: bool = False,
                       leaf_obs: bool = False, _expand=None):
        """Score C candidate plans from the live batch without touching it (Handle.evaluate_plans):
        actions [T, C, N, 2], roots [C] (the live env each candidate starts from; C is free of
        num_envs) -> dict of returns [C, N] (discounted by gamma, f32), reward_seq / done_seq /
        status_seq [T, C, N] (zero after a candidate stopped), substeps / terminated / truncated [C].
        No observation and no LiDAR: run the winner through `step_sequence` for its leaf.  The env's
        state, last outputs and random stream stay as they are.  spawn_route, if given, is [T][C].
        torch: stream-ordered on the current stream, zero-copy; the returned tensors are cached per
        (T, C) and reused by the next call of that shape.
        leaf_obs=True (mev_evaluate_leaves): the dict gains leaf_obs [C, N, obs_dim], the observation
        of the state every candidate stopped at -- for planners that add a value at the leaf."""
        if self.backend == "torch":
            t = self._torch
            self._bind_stream()
            a, r = self._dev_tensor(actions, t.float32), self._dev_tensor(roots, t.int32)
            if r.dim() != 1 or a.dim() != 4 or tuple(a.shape[1:]) != (r.shape[0], self.num_agents, 2):
                raise ValueError(f"actions must be [T, C, {self.num_agents}, 2] and roots [C], got {tuple(a.shape)} "
                                 f"and {tuple(r.shape)}")
            T, C = int(a.shape[0]), int(r.shape[0])
            o = self._eval_out(T, C, leaf_obs)
            sp = None
            if spawn_route is not None:
                sp = self._dev_tensor(spawn_route, t.int32)
                if tuple(sp.shape) != (T, C):
                    raise ValueError(f"spawn_route must be [{T}][{C}], got {tuple(sp.shape)}")
            if _expand is not None:
                d = self._dev_tensor(_expand["dst_slots"], t.int32)
                if tuple(d.shape) != (C,):
                    raise ValueError(f"dst_slots must be [{C}], got {tuple(d.shape)}")
                self._h.expand_plans(a, r, _expand["dst"], d, _expand["src"], _expand["counter_offset"], leaf_obs, dt,
                                     gamma, spawn_route=sp, out=o, device=True, candidates=C, length=T)
            else:
                self._h.evaluate_plans(a, r, dt, gamma, spawn_route=sp, out=o, device=True, candidates=C, length=T,
                                       leaf_obs=leaf_obs)
            return {k: v.clone() for k, v in o.items()} if copy else o
        shape = np.shape(actions)
        if len(shape) != 4:
            raise ValueError(f"actions must be [T, C, {self.num_agents}, 2], got {shape}")
        o = self._eval_out(int(shape[0]), int(shape[1]), leaf_obs)
        if _expand is not None:
            self._h.expand_plans(actions, roots, _expand["dst"], _expand["dst_slots"], _expand["src"],
                                 _expand["counter_offset"], leaf_obs, dt, gamma, spawn_route=spawn_route, out=o)
        else:
            self._h.evaluate_plans(actions, roots, dt, gamma, spawn_route=spawn_route, out=o, leaf_obs=leaf_obs)
        return {k: v.copy() for k, v in o.items()} if copy else o

    def make_pool(self, slots: int):
        """A state pool of `slots` slots on this env's handle (Handle.pool): where expand_plans keeps
        the states its candidates stop at, and where deeper expansions start from."""
        return self._h.pool(slots)

    def expand_plans(self, actions, roots, dst, dst_slots, src=None, counter_offset: int = 0, leaf_obs: bool = False,
                     dt=1.0 / 60.0, gamma: float = 1.0, spawn_route=None, copy: bool = False):
        """evaluate_plans whose candidates start from slots roots[c] of pool `src` (None: from live
        envs) and whose stop states go to slots dst_slots[c] of pool `dst` (-1: not stored) --
        Handle.expand_plans.  The same dict, buffers and stream rules as evaluate_plans; the env's
        state, last outputs and random stream stay as they are."""
        return self.evaluate_plans(actions, roots, dt, gamma, spawn_route, copy, leaf_obs,
                                   _expand=dict(dst=dst, dst_slots=dst_slots, src=src, counter_offset=counter_offset))

    def sample_plans(self, mean, sigma, roots, samples: int, dt=1.0 / 60.0, gamma: float = 1.0, lo=(-1.0, -1.0),
                     hi=(1.0, 1.0), seed: int = 0, counter: int = 0, mean_first: bool = False, leaf_obs: bool = False,
                     spawn_route=None, copy: bool = False, src=None, dst=None, dst_slots=None, counter_offset: int = 0):
        """evaluate_plans whose C = G * samples candidates draw their own actions on the device
        (Handle.sample_plans): mean, sigma [T, G, N, 2], roots [G] -> evaluate_plans' dict plus
        actions_out [T, C, N, 2], the clamped actions the candidates ran.  The noise is the stated
        Irwin-Hall approximation of a unit Gaussian from the Philox stream (seed, counter): pass a
        new counter per iteration.  The same buffers (kept per (T, C)) and stream rules as
        evaluate_plans; the env's state, last outputs and random stream stay as they are.
        dst (mev_sample_expand_plans): the stop states go to slots dst_slots[c] ([C]; -1: not stored)
        of pool `dst` and the groups start from slots roots[g] of pool `src` (None: from live envs),
        as in expand_plans -- with dst_slots[c] = c, update_plans' `order` names the next level's
        roots.  src or dst_slots without dst: ValueError."""
        K, N = int(samples), self.num_agents
        if dst is None and (src is not None or dst_slots is not None):
            raise ValueError("src and dst_slots need dst (the pool that receives the stop states)")
        pool = dict(src=src, dst=dst, dst_slots=dst_slots, counter_offset=counter_offset)
        if self.backend == "torch":
            t = self._torch
            self._bind_stream()
            m, s, r = self._dev_tensor(mean, t.float32), self._dev_tensor(sigma, t.float32), self._dev_tensor(roots, t.int32)
            if r.dim() != 1 or m.dim() != 4 or tuple(m.shape[1:]) != (r.shape[0], N, 2) or s.shape != m.shape:
                raise ValueError(f"mean and sigma must be [T, G, {N}, 2] and roots [G], got {tuple(m.shape)}, "
                                 f"{tuple(s.shape)} and {tuple(r.shape)}")
            T, G = int(m.shape[0]), int(r.shape[0])
            o = self._sample_out(T, G * K, leaf_obs)
            sp = None
            if spawn_route is not None:
                sp = self._dev_tensor(spawn_route, t.int32)
                if tuple(sp.shape) != (T, G * K):
                    raise ValueError(f"spawn_route must be [{T}][{G * K}], got {tuple(sp.shape)}")
            if dst_slots is not None:
                pool["dst_slots"] = self._dev_tensor(dst_slots, t.int32)
                if tuple(pool["dst_slots"].shape) != (G * K,):
                    raise ValueError(f"dst_slots must be [{G * K}], got {tuple(pool['dst_slots'].shape)}")
            self._h.sample_plans(m, s, r, K, dt, gamma, lo, hi, seed, counter, mean_first, leaf_obs, sp, out=o,
                                 device=True, groups=G, length=T, **pool)
            return {k: v.clone() for k, v in o.items()} if copy else o
        shape = np.shape(mean)
        if len(shape) != 4:
            raise ValueError(f"mean must be [T, G, {N}, 2], got {shape}")
        o = self._sample_out(int(shape[0]), int(shape[1]) * K, leaf_obs)
        self._h.sample_plans(mean, sigma, roots, K, dt, gamma, lo, hi, seed, counter, mean_first, leaf_obs, spawn_route,
                             out=o, **pool)
        return {k: v.copy() for k, v in o.items()} if copy else o

    def _sample_out(self, T, C, leaf):
        """evaluate_plans' buffers of (T, C) with the actions_out buffer of that shape beside them."""
        o = self._eval_out(T, C, leaf)
        ao = self._out_eval.get((T, C, "actions"))
        if ao is None:
            shape = (T, C, self.num_agents, 2)
            if self.backend == "torch":
                ao = self._torch.zeros(shape, dtype=self._torch.float32, device=self._out["obs"].device)
            else:
                ao = np.zeros(shape, np.float32)
            self._out_eval[(T, C, "actions")] = ao
        return dict(o, actions_out=ao)

    @staticmethod
    def _policy_activations(module):
        """(hidden, out) of an nn.Sequential(Linear, A, Linear[, A, Linear][, Tanh]): A is ReLU or Tanh, the same
        at every hidden layer -> "relu" | "tanh"; a trailing Tanh is the output activation -> "tanh", else
        "linear".  ValueError for any other module, and for Sequential(Linear, Tanh, Linear) -- one tanh hidden
        layer and a raw mean -- which make_policy has always refused and takes as arrays with hidden="tanh"."""
        layers = list(module.children())
        names = [type(x).__name__ for x in layers]
        out = "linear"
        if len(layers) in (4, 6) and names[-1] == "Tanh":
            out, layers, names = "tanh", layers[:-1], names[:-1]
        shape = "nn.Sequential(Linear, A, Linear[, A, Linear][, Tanh]) with biases, A = ReLU or Tanh"
        if not (len(layers) in (3, 5) and all(n == "Linear" and x.bias is not None for n, x in zip(names[0::2], layers[0::2]))
                and all(n in ("ReLU", "Tanh") for n in names[1::2])):
            raise ValueError(f"a policy module is {shape}")
        if len(set(names[1::2])) != 1:
            raise ValueError(f"a policy module is {shape}: the hidden activation A must be the same at every hidden "
                             f"layer, got {names[1::2]}")
        hidden = "tanh" if names[1] == "Tanh" else "relu"
        if hidden == "tanh" and out == "linear" and len(layers) == 3:
            # Sequential(Linear, Tanh, Linear) was refused before tanh policies existed, and that refusal is part of
            # what callers and the suite rely on (a module that is silently not the ReLU network it was taken for)
            raise ValueError("nn.Sequential(Linear, Tanh, Linear) is not taken from a module: pass its arrays, "
                             'make_policy((weights, biases), hidden="tanh")')
        return hidden, out

    @staticmethod
    def _policy_arrays(module_or_arrays):
        """(weights, biases) of an nn.Sequential(Linear, A, Linear[, A, Linear][, Tanh]) (_policy_activations) --
        its parameters' own tensors -- or of a (weights, biases) pair of array lists."""
        m = module_or_arrays
        if hasattr(m, "children"):
            VecIntersectionEnv._policy_activations(m)
            lin = [x for x in m.children() if type(x).__name__ == "Linear"]
            return [x.weight for x in lin], [x.bias for x in lin]
        weights, biases = m
        return list(weights), list(biases)

    def _policy_inputs(self, module_or_arrays):
        weights, biases = self._policy_arrays(module_or_arrays)
        if self.backend != "torch":
            host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else x
            return [host(w) for w in weights], [host(b) for b in biases], False
        self._bind_stream()
        t = self._torch
        dev = lambda x: self._dev_tensor(x.detach() if hasattr(x, "detach") else x, t.float32)
        return [dev(w) for w in weights], [dev(b) for b in biases], True

    def _value_inputs(self, value):
        """(w, b, device) of a value head: an nn.Linear(H_last, 1) -- its parameters' own tensors -- or a (w, b) pair."""
        w, b = (value.weight, value.bias) if hasattr(value, "weight") else value
        if b is None:
            raise ValueError("a value head is nn.Linear(H_last, 1) with a bias, or a (w, b) pair")
        if self.backend != "torch":
            host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else x
            return host(w), host(b), False
        self._bind_stream()
        t = self._torch
        dev = lambda x: self._dev_tensor(x.detach() if hasattr(x, "detach") else x, t.float32)
        return dev(w), dev(b), True

    def make_policy(self, module_or_arrays, value=None, hidden=None, out=None):
        """An MLP policy on the device (Handle.policy) from an nn.Sequential(Linear, A, Linear[, A, Linear][,
        Tanh]) or a (weights, biases) pair of array lists ([out][in] and [out]; the last layer has 2
        outputs: throttle, steer).  A is nn.ReLU or nn.Tanh, the same at every hidden layer (the stock 64-64 tanh
        PPO actor); a trailing nn.Tanh squashes the mean before noise and clamp (DDPG / TD3 actors).  The tanh is
        tanh_c, the library's stated f32 tanh (_capi.tanh_c), within 2 ulp of the exact one.  One shape is not taken
        from a module, as before: Sequential(Linear, Tanh, Linear) -- pass its arrays with hidden="tanh".  With arrays the
        keywords hidden ("relu" | "tanh") and out ("linear" | "tanh") say the same; with a module they must agree
        with it where given.  The activations are fixed at creation: refresh keeps them.  value: a critic head on the same trunk, nn.Linear(H_last, 1) or a (w, b)
        pair ([H_last] or [1][H_last], and [1]); `rollout` can then return value_seq.
        `policy.refresh(module_or_arrays, value)` pushes new weights of the same shape, the head's included.
        torch backend: the weights are read on the current stream by a small kernel, no host copy, no sync."""
        if hasattr(module_or_arrays, "children"):
            mh, mo = self._policy_activations(module_or_arrays)
            if hidden not in (None, mh) or out not in (None, mo):
                raise ValueError(f"the module's activations are hidden={mh!r}, out={mo!r}; got hidden={hidden!r}, out={out!r}")
            hidden, out = mh, mo
        hidden, out = hidden or "relu", out or "linear"
        w, b, device = self._policy_inputs(module_or_arrays)
        pol = self._h.policy(w, b, device=device, hidden=hidden, out=out)
        if value is not None:
            vw, vb, device = self._value_inputs(value)
            pol.set_value_head(vw, vb, device=device)

        def refresh(source=module_or_arrays, value=value):
            if hasattr(source, "children") and self._policy_activations(source) != (hidden, out):
                raise ValueError(f"refresh: the policy's activations are fixed at creation (hidden={hidden!r}, out={out!r})")
            w, b, device = self._policy_inputs(source)
            pol.update(w, b, device=device)
            if value is not None:
                vw, vb, device = self._value_inputs(value)
                pol.set_value_head(vw, vb, device=device)

        pol.refresh = refresh
        return pol

    def rollout(self, policy, T: int, dt: float = 1.0 / 60.0, sigma=None, lo=(-1.0, -1.0), hi=(1.0, 1.0), seed: int = 0,
                counter: int = 0, spawn_route=None, outputs=_capi.ROLLOUT_OUTPUTS, copy: bool = False, repeat: int = 1,
                assign=None):
        """T steps of observe -> policy -> step in one launch (Handle.rollout_policy), auto-reset as this env
        was made: a dict of obs_seq [T, E, N, obs_dim] (the observation after each sub-step), actions_seq,
        mean_seq [T, E, N, 2], reward_seq, done_seq, status_seq [T, E, N], terminated_seq, truncated_seq
        [T, E] -- those named in `outputs`.  sigma: None, or two floats for Gaussian-like exploration noise
        from the Philox stream (seed, counter): pass a new counter per call.  torch backend: device tensors
        (kept per (T, outputs) and rewritten by the next call unless copy=True), stream-ordered, no host sync.
        With "value_seq" among the outputs (a policy made with value=...): value_seq [T + 1, E, N], V of the
        observation before each sub-step and of the last one, and `ended_before` [E], whether the env's step
        before this call ended it -- the dict is what `gae` takes.
        repeat = n > 1 (Handle.rollout_policy's): T decisions, each action held for up to n sub-steps as
        `step` holds it with frame_skip=n -- rewards summed, done and status latched, one LiDAR cast, the env
        stopping at its end; every row is a decision's, spawn_route is [T, repeat, E], and "substeps_seq"
        among the outputs gives the sub-steps each decision ran [T, E] (int32).  `repeat` does NOT default to
        the constructor's frame_skip -- this call never repeated -- so pass repeat=env.frame_skip to roll out
        as `step` steps.  `gae` on such a dict applies gamma and lambda per decision.
        A policy per agent slot (Handle.rollout_policies): `policy` a list or tuple of up to 8 policies of
        `make_policy` and `assign` uint8 [E, N], or [N] for the same seats in every env -- slot (e, i) is driven by
        policy[assign[e, i]] for the whole call, across respawns and auto-resets; sigma is then None or [P, 2], a
        row per policy, "value_seq" needs a value head on every listed policy, and spawn_route is
        [T, repeat, E].  `gae` takes the dict as it is; mask the loss to the learner's slots (assign == its index)."""
        T, repeat = int(T), int(repeat)
        multi = isinstance(policy, (list, tuple))
        if multi != (assign is not None):
            raise ValueError("a list or tuple of policies goes with `assign`, a single policy without it")
        key = (T, tuple(outputs), "rollout")
        o = self._out_eval.get(key)
        values = "value_seq" in outputs
        outs = _capi._ROLLOUT_OUTS + ((_capi._VALUE_OUT,) if values else ()) + (_capi._SUBSTEPS_OUT,)
        held = repeat != 1 or "substeps_seq" in outputs or multi
        route_shape = (T, repeat, self.num_envs) if held else (T, self.num_envs)

        def call(route, **kw):
            if not multi:
                return self._h.rollout_policy(policy, T, dt, sigma, lo, hi, seed, counter, self.auto_reset, route,
                                              repeat=repeat, **kw)
            if self.backend == "torch":
                a = self._dev_tensor(assign, self._torch.uint8)
                a = a.expand(self.num_envs, self.num_agents).contiguous() if a.dim() == 1 else a
                if tuple(a.shape) != (self.num_envs, self.num_agents):
                    raise ValueError(f"assign must be [E, N] or [N], got {tuple(a.shape)}")
            else:
                a = np.asarray(assign)
                a = np.broadcast_to(a, (self.num_envs, self.num_agents)) if a.ndim == 1 else a
                a = np.ascontiguousarray(a, np.uint8)
            return self._h.rollout_policies(policy, a, T, dt, sigma, lo, hi, seed, counter, self.auto_reset, route,
                                            repeat=repeat, **kw)

        if self.backend == "torch":
            t = self._torch
            self._bind_stream()
            if o is None:
                o = self._out_eval[key] = {}
                E, N, D = self.num_envs, self.num_agents, self.obs_dim
                for k, dtype, shape in outs:
                    if k in outputs:
                        tdt = t.float32 if dtype is np.float32 else t.int32 if dtype is np.int32 else t.uint8
                        o[k] = t.zeros(shape(T, E, N, D), dtype=tdt, device=self._out["obs"].device)
            sp = None
            if spawn_route is not None:
                sp = self._dev_tensor(spawn_route, t.int32)
                if tuple(sp.shape) != route_shape:
                    raise ValueError(f"spawn_route must be {list(route_shape)}, got {tuple(sp.shape)}")
            eb = None
            if values:  # (read on the stream before the call rewrites the handle's last outputs; a fresh tensor)
                last = {k: t.empty(self.num_envs, dtype=t.uint8, device=self._out["obs"].device)
                        for k in ("terminated", "truncated")}
                self._h.get_outputs(last, device=True)
                eb = last["terminated"] | last["truncated"]
            call(sp, out=o, device=True)
            r = {k: v.clone() for k, v in o.items()} if copy else dict(o)
            if values:
                r["ended_before"] = eb
            return r
        if o is None:
            E, N, D = self.num_envs, self.num_agents, self.obs_dim
            o = self._out_eval[key] = {k: np.zeros(shape(T, E, N, D), dtype) for k, dtype, shape in outs if k in outputs}
        eb = None
        if values:
            last = self._h.get_outputs()
            eb = ((last["terminated"] != 0) | (last["truncated"] != 0)).astype(np.uint8)
        call(spawn_route, out=o)
        r = {k: v.copy() for k, v in o.items()} if copy else dict(o)
        if values:
            r["ended_before"] = eb
        return r

    def gae(self, traj, gamma: float = 0.99, lam: float = 0.95, mask_reset_steps: bool = True):
        """Advantages of a `rollout` dict that holds reward_seq and value_seq (Handle.gae): done_seq,
        terminated_seq, truncated_seq and ended_before are used where the dict has them.  Returns
        `advantages`, `returns` and `valid` [T, E, N]; with mask_reset_steps the transitions that follow an
        env's end (this env's auto-reset steps, whose action came from the terminal observation) get
        advantage 0 and valid 0.  Fresh arrays every call; torch: stream-ordered, no host sync.
        On a `rollout(..., repeat=n)` dict the rows are decisions: gamma and lambda then apply per decision."""
        names = ("done_seq", "terminated_seq", "truncated_seq", "ended_before")
        opt = {k: traj.get(k) for k in names}
        outputs = ("advantages", "returns", "valid")
        if self.backend != "torch":
            return self._h.gae(traj["reward_seq"], traj["value_seq"], gamma=gamma, lam=lam,
                               mask_reset_steps=mask_reset_steps, outputs=outputs, **opt)
        t = self._torch
        self._bind_stream()
        opt = {k: None if v is None else self._dev_tensor(v, t.uint8) for k, v in opt.items()}
        return self._h.gae(self._dev_tensor(traj["reward_seq"], t.float32), self._dev_tensor(traj["value_seq"], t.float32),
                           gamma=gamma, lam=lam, mask_reset_steps=mask_reset_steps, outputs=outputs, device=True, **opt)

    def update_plans(self, actions, samples: int, scores=None, returns=None, mode: str = "elites", elites=None,
                     temperature: float = 1.0, sigma_min: float = 0.0):
        """Rank each group's candidates and refit the sampling distribution (Handle.update_plans):
        actions [T, G * samples, N, 2] (sample_plans' actions_out), scores [C] or returns [C, N] ->
        dict of new_mean / new_sigma [T, G, N, 2] (the next sample_plans' input), best / best_score
        [G] and order [G, elites] ("elites") or weights [C] ("softmax").  Fresh arrays every call;
        torch: stream-ordered on the current stream, no synchronisation."""
        K, N = int(samples), self.num_agents
        if self.backend != "torch":
            return self._h.update_plans(actions, K, scores, returns, mode, elites, temperature, sigma_min)
        t = self._torch
        self._bind_stream()
        a = self._dev_tensor(actions, t.float32)
        if a.dim() != 4 or tuple(a.shape[2:]) != (N, 2) or a.shape[1] % K:
            raise ValueError(f"actions must be [T, G * {K}, {N}, 2], got {tuple(a.shape)}")
        T, C = int(a.shape[0]), int(a.shape[1])
        G = C // K
        sc = None if scores is None else self._dev_tensor(scores, t.float32)
        rt = None if returns is None else self._dev_tensor(returns, t.float32)
        if (sc is not None and tuple(sc.shape) != (C,)) or (rt is not None and tuple(rt.shape) != (C, N)):
            raise ValueError(f"scores must be [{C}] and returns [{C}, {N}]")
        M = int(elites) if elites is not None else max(1, K // 4)
        dev = a.device
        o = {"new_mean": t.empty((T, G, N, 2), dtype=t.float32, device=dev),
             "new_sigma": t.empty((T, G, N, 2), dtype=t.float32, device=dev),
             "best": t.empty((G,), dtype=t.int32, device=dev), "best_score": t.empty((G,), dtype=t.float32, device=dev)}
        if mode == "elites":
            o["order"] = t.empty((G, M), dtype=t.int32, device=dev)
        else:
            o["weights"] = t.empty((C,), dtype=t.float32, device=dev)
        self._h.update_plans(a, K, sc, rt, mode, M, temperature, sigma_min, out=o, device=True, groups=G, length=T)
        return o

    def _eval_out(self, T, C, leaf=False):
        """The output buffers of evaluate_plans, kept per (T, C); leaf: with the leaf_obs buffer of
        that shape (made at the first call that asks for it; the default call's dict never has it)."""
        if not 1 <= T <= _capi.MEV_MAX_REPEAT or not 1 <= C <= _capi.MEV_MAX_CANDIDATES:
            raise ValueError(f"a call has 1..{_capi.MEV_MAX_REPEAT} rows and 1..{_capi.MEV_MAX_CANDIDATES} candidates, "
                             f"got {T} and {C}")
        o = self._out_eval.get((T, C))
        if o is None:
            o = {}
            for k, dtype, shape in _capi._EVAL_OUTS:
                if self.backend == "torch":
                    o[k] = self._torch.zeros(shape(T, C, self.num_agents), dtype=getattr(self._torch, np.dtype(dtype).name),
                                             device=self._out["obs"].device)
                else:
                    o[k] = np.zeros(shape(T, C, self.num_agents), dtype)
            self._out_eval[(T, C)] = o
        if leaf:
            lo = self._out_eval.get((T, C, "leaf"))
            if lo is None:
                shape = (C, self.num_agents, int(self._out["obs"].shape[-1]))
                if self.backend == "torch":
                    lo = self._torch.zeros(shape, dtype=self._torch.float32, device=self._out["obs"].device)
                else:
                    lo = np.zeros(shape, np.float32)
                self._out_eval[(T, C, "leaf")] = lo
            o = dict(o, leaf_obs=lo)
        return o

    def _actions_tensor(self, actions, plan):
        """actions as a contiguous float32 tensor on this env's device: [E, N, 2], or (plan) [T, E, N, 2]."""
        t = self._torch
        a = actions
        if not (isinstance(a, t.Tensor) and a.is_cuda and a.dtype == t.float32 and a.is_contiguous()):
            a = t.as_tensor(a, dtype=t.float32, device=self._out["obs"].device).contiguous()
        if (plan and a.dim() < 2) or a.numel() != (a.shape[0] if plan else 1) * self.num_envs * self.num_agents * 2:
            raise ValueError(f"actions must be [{'T, ' if plan else ''}{self.num_envs}, {self.num_agents}, 2], "
                             f"got {tuple(a.shape)}")
        if a.device.index != self.device_index:
            raise ValueError("actions are on another device")
        return a

    def _spawn_tensor(self, spawn_route, rows=None):
        """spawn_route (or None) as a contiguous int32 tensor on this env's device; rows: it must be [rows][E]."""
        if spawn_route is None:
            return None
        sp = self._torch.as_tensor(spawn_route, dtype=self._torch.int32, device=self._out["obs"].device).contiguous()
        if rows is not None and tuple(sp.shape) != (rows, self.num_envs):
            raise ValueError(f"spawn_route must be [{rows}][{self.num_envs}], got {tuple(sp.shape)}")
        return sp

    def _window_out(self, T=None):
        """The step's output buffers plus substeps (made at the first window) and, for a plan of T
        rows, the [T, E, N] per-step rows (kept per T)."""
        if T is not None and not 1 <= T <= _capi.MEV_MAX_REPEAT:
            raise ValueError(f"a plan has 1..{_capi.MEV_MAX_REPEAT} rows, got {T}")
        def zeros(shape, dtype):
            if self.backend == "torch":
                return self._torch.zeros(shape, dtype=getattr(self._torch, dtype), device=self._out["obs"].device)
            return np.zeros(shape, dtype)

        if self._out_rep is None:
            self._out_rep = dict(self._out, substeps=zeros(self.num_envs, "int32"))
        if T is None:
            return self._out_rep
        if self._out_seq is None or self._out_seq["reward_seq"].shape[0] != T:
            shape = (T, self.num_envs, self.num_agents)
            self._out_seq = dict(self._out_rep, reward_seq=zeros(shape, "float32"), done_seq=zeros(shape, "uint8"),
                                 status_seq=zeros(shape, "uint8"))
        return self._out_seq

    def observations(self):
        return self._out["obs"]

    def get_state(self) -> Dict[str, np.ndarray]:
        if self.backend == "torch":
            self._torch.cuda.current_stream(self.device_index).synchronize()
        return self._h.get_state()

    def set_state(self, state: Dict[str, np.ndarray]):
        self._h.set_state(state)

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_default_routes(num_agents: int, num_lanes: int):
    """Ego routes as env.py assigns them (mapping order, wrapping; reference env.py:138-145)."""
    table = default_routes(num_lanes)
    return [table[i % len(table)] for i in range(num_agents)]
