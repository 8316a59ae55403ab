"""ctypes binding of libmarlenv_hip.so (include/marlenv.h).

The product path: every simulator computation happens in the gfx950 library;
this module only marshals buffers.  Importing works without a GPU (the CPU
test-suite checks the exported symbols), but creating a handle requires the
HIP runtime and a device — there is NO CPU fallback: a missing library or
device raises.
"""
from __future__ import annotations

import ctypes
import operator
import os
from typing import Dict, Optional

import numpy as np

from . import _build

LIB_PATH = _build.LIB_PATH

MEV_DEVICE_PTRS = 0x1
MEV_AUTO_RESET = 0x2
MEV_GATHER_TO_ROOT = 0x4
MEV_POLICY_HIDDEN_TANH = 0x10  # mev_policy_create: tanh_c hidden layers
MEV_POLICY_OUT_TANH = 0x20     # mev_policy_create: mu = tanh_c(mu)
MEV_COMM_ID_BYTES = 128
MEV_GATHER_F32 = 0
MEV_GATHER_LIDAR_U8 = 1
MEV_GATHER_STATE = 2
STATE_BYTES_PER_AGENT = 22
# packed-output fields (mev_packed_layout2) and DLPack outputs (mev_output_dlpack), include/marlenv.h order
PACKED_FIELDS = ("obs", "reward", "done", "status", "terminated", "truncated", "lidar", "state")
DLPACK_OUTPUTS = ("obs", "reward", "done", "status", "terminated", "truncated", "agents_alive", "step", "gathered")

STATUS_NAMES = ("ALIVE", "DEAD", "SUCCESS", "CRASH_WALL", "CRASH_LINE", "CRASH_CAR")
PATH_LEN = 160  # every lane-layout route
MAX_PATH_LEN = 4096  # a written path (mev_add_route_n)

# exported symbols that include/marlenv.h declares (checked by tests/test_capi_symbols.py)
EXPORTED = (
    "mev_last_error", "mev_abi_version", "mev_device_count", "mev_config_default", "mev_create", "mev_destroy",
    "mev_get_config", "mev_obs_dim", "mev_set_stream", "mev_sync", "mev_num_points", "mev_point_xy",
    "mev_route_id", "mev_route_info", "mev_route_len", "mev_path_len", "mev_set_ego_routes", "mev_set_traffic_routes",
    "mev_default_traffic_routes", "mev_reset", "mev_step", "mev_step_repeat", "mev_get_outputs", "mev_get_state", "mev_set_state",
    "mev_device_outputs", "mev_npc_overflow", "mev_npc_stats", "mev_use_own_stream", "mev_debug_stamps",
    "mev_configure", "mev_configure_traffic", "mev_set_reward", "mev_car_update", "mev_car_check_collision",
    "mev_kernel_timing", "mev_kernel_times", "mev_set_reset_routes", "mev_snapshot_size", "mev_snapshot",
    "mev_restore", "mev_set_step_kernel", "mev_get_step_kernel", "mev_set_step_pack", "mev_get_step_pack",
    "mev_set_step_split", "mev_get_step_split", "mev_set_env_deal", "mev_set_serve", "mev_serve_stats",
    "mev_packed_layout", "mev_comm_unique_id", "mev_comm_init", "mev_comm_destroy", "mev_gather_result",
    "mev_gather_wait", "mev_output_dlpack", "mev_packed_layout2", "mev_set_gather_format", "mev_lidar_decode_table",
    "mev_unpack_gathered", "mev_add_route", "mev_add_route_n", "mev_set_car_dims", "mev_get_car_dims", "mev_car_dims_active",
    "mev_set_beam_angles", "mev_get_beam_angles", "mev_decode_errors", "mev_step_sequence", "mev_restore_map",
    "mev_evaluate_plans", "mev_evaluate_leaves", "mev_pool_create", "mev_pool_destroy", "mev_pool_slots",
    "mev_pool_capture", "mev_pool_get_state", "mev_expand_plans", "mev_sample_plans", "mev_update_plans",
    "mev_sample_expand_plans", "mev_get_step_row", "mev_policy_create", "mev_policy_update", "mev_policy_destroy",
    "mev_rollout_policy", "mev_get_rollout_row", "mev_policy_set_value_head", "mev_policy_has_value_head",
    "mev_rollout_policy_values", "mev_gae", "mev_rollout_policy_repeat", "mev_rollout_policies",
    "mev_tanh", "mev_policy_get_activations",
)


class MevConfig(ctypes.Structure):
    _fields_ = [
        ("num_envs", ctypes.c_int32), ("num_agents", ctypes.c_int32), ("num_lanes", ctypes.c_int32),
        ("lidar_rays", ctypes.c_int32), ("lidar_fov_deg", ctypes.c_float), ("lidar_max_dist", ctypes.c_float),
        ("lidar_step", ctypes.c_float), ("obs_dim", ctypes.c_int32), ("traffic_flow", ctypes.c_int32),
        ("traffic_density", ctypes.c_float), ("use_team_reward", ctypes.c_int32), ("respawn_enabled", ctypes.c_int32),
        ("max_steps", ctypes.c_int32), ("reward", ctypes.c_float * 8), ("max_npcs", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("device", ctypes.c_int32),
    ]


_vp = ctypes.c_void_p


class MevStepArgs(ctypes.Structure):
    _fields_ = [
        ("actions", _vp), ("dt", ctypes.c_float), ("spawn_route", _vp), ("obs", _vp), ("reward", _vp),
        ("done", _vp), ("status", _vp), ("terminated", _vp), ("truncated", _vp), ("agents_alive", _vp),
        ("step", _vp), ("flags", ctypes.c_uint32),
    ]


MEV_MAX_REPEAT = 64


class MevRepeatArgs(ctypes.Structure):
    _fields_ = [("step", MevStepArgs), ("repeat", ctypes.c_int32), ("substeps", _vp)]


class MevSequenceArgs(ctypes.Structure):  # mev_sequence_args
    _fields_ = [("step", MevStepArgs), ("length", ctypes.c_int32), ("dt_seq", ctypes.POINTER(ctypes.c_float)),
                ("reward_seq", _vp), ("done_seq", _vp), ("status_seq", _vp), ("substeps", _vp)]


_SEQ_KEYS = ("reward_seq", "done_seq", "status_seq")

MEV_MAX_CANDIDATES = 1 << 20


class MevEvaluateArgs(ctypes.Structure):  # mev_evaluate_args
    _fields_ = [("actions", _vp), ("roots", _vp), ("spawn_route", _vp), ("candidates", ctypes.c_int32),
                ("length", ctypes.c_int32), ("dt", ctypes.c_float), ("dt_seq", ctypes.POINTER(ctypes.c_float)),
                ("gamma", ctypes.c_float), ("returns", _vp), ("reward_seq", _vp), ("done_seq", _vp),
                ("status_seq", _vp), ("substeps", _vp), ("terminated", _vp), ("truncated", _vp),
                ("flags", ctypes.c_uint32)]


class MevLeafArgs(ctypes.Structure):  # mev_leaf_args
    _fields_ = [("eval", MevEvaluateArgs), ("leaf_obs", _vp)]


MEV_MAX_POOL_SLOTS = 1 << 20


class MevExpandArgs(ctypes.Structure):  # mev_expand_args
    _fields_ = [("eval", MevEvaluateArgs), ("leaf_obs", _vp), ("src", _vp), ("dst", _vp), ("dst_slots", _vp),
                ("counter_offset", ctypes.c_uint64)]


MEV_SAMPLE_MEAN_FIRST = 0x1
MEV_UPDATE_ELITES, MEV_UPDATE_SOFTMAX = 0, 1
MEV_MAX_SAMPLES = 4096


class MevSampleArgs(ctypes.Structure):  # mev_sample_args
    _fields_ = [("eval", MevEvaluateArgs), ("leaf_obs", _vp), ("mean", _vp), ("sigma", _vp),
                ("lo", ctypes.c_float * 2), ("hi", ctypes.c_float * 2), ("groups", ctypes.c_int32),
                ("samples", ctypes.c_int32), ("noise_seed", ctypes.c_uint64), ("noise_counter", ctypes.c_uint64),
                ("actions_out", _vp), ("sample_flags", ctypes.c_uint32)]


class MevSampleExpandArgs(ctypes.Structure):  # mev_sample_expand_args
    _fields_ = [("sample", MevSampleArgs), ("src", _vp), ("dst", _vp), ("dst_slots", _vp),
                ("counter_offset", ctypes.c_uint64)]


class MevUpdateArgs(ctypes.Structure):  # mev_update_args
    _fields_ = [("actions", _vp), ("scores", _vp), ("returns", _vp), ("groups", ctypes.c_int32),
                ("samples", ctypes.c_int32), ("length", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("elites", ctypes.c_int32), ("inv_temperature", ctypes.c_float), ("sigma_min", ctypes.c_float),
                ("new_mean", _vp), ("new_sigma", _vp), ("best", _vp), ("best_score", _vp), ("order", _vp),
                ("weights", _vp), ("flags", ctypes.c_uint32)]


MEV_POLICY_MAX_WIDTH = 128
MEV_MAX_ROLLOUT = 1024


class MevPolicySpec(ctypes.Structure):  # mev_policy_spec
    _fields_ = [("in_dim", ctypes.c_int32), ("hidden", ctypes.c_int32 * 2), ("w", _vp * 3), ("b", _vp * 3)]


class MevRolloutArgs(ctypes.Structure):  # mev_rollout_args
    _fields_ = [("policy", _vp), ("length", ctypes.c_int32), ("dt", ctypes.c_float), ("spawn_route", _vp),
                ("sigma", ctypes.POINTER(ctypes.c_float)), ("lo", ctypes.c_float * 2), ("hi", ctypes.c_float * 2),
                ("noise_seed", ctypes.c_uint64), ("noise_counter", ctypes.c_uint64), ("obs_seq", _vp),
                ("actions_seq", _vp), ("mean_seq", _vp), ("reward_seq", _vp), ("done_seq", _vp), ("status_seq", _vp),
                ("terminated_seq", _vp), ("truncated_seq", _vp), ("flags", ctypes.c_uint32)]


class MevRolloutValuesArgs(ctypes.Structure):  # mev_rollout_values_args
    _fields_ = [("rollout", MevRolloutArgs), ("value_seq", _vp)]


MEV_MAX_ROLLOUT_SUBSTEPS = 4096


class MevRolloutRepeatArgs(ctypes.Structure):  # mev_rollout_repeat_args
    _fields_ = [("rollout", MevRolloutArgs), ("value_seq", _vp), ("repeat", ctypes.c_int32), ("substeps_seq", _vp)]


MEV_MAX_ROLLOUT_POLICIES = 8


class MevRolloutMultiArgs(ctypes.Structure):  # mev_rollout_multi_args
    _fields_ = [("base", MevRolloutRepeatArgs), ("policies", ctypes.POINTER(_vp)), ("count", ctypes.c_int32),
                ("assign", _vp), ("sigma", ctypes.POINTER(ctypes.c_float))]


MEV_GAE_MASK_RESET_STEPS = 0x100


class MevGaeArgs(ctypes.Structure):  # mev_gae_args
    _fields_ = [("reward_seq", _vp), ("value_seq", _vp), ("done_seq", _vp), ("terminated_seq", _vp),
                ("truncated_seq", _vp), ("ended_before", _vp), ("length", ctypes.c_int32), ("gamma", ctypes.c_float),
                ("lam", ctypes.c_float), ("advantages", _vp), ("returns", _vp), ("valid", _vp),
                ("flags", ctypes.c_uint32)]


# outputs of rollout_policy: (key, dtype, shape of (T, E, N, D))
_ROLLOUT_OUTS = (("obs_seq", np.float32, lambda T, E, N, D: (T, E, N, D)),
                 ("actions_seq", np.float32, lambda T, E, N, D: (T, E, N, 2)),
                 ("mean_seq", np.float32, lambda T, E, N, D: (T, E, N, 2)),
                 ("reward_seq", np.float32, lambda T, E, N, D: (T, E, N)),
                 ("done_seq", np.uint8, lambda T, E, N, D: (T, E, N)),
                 ("status_seq", np.uint8, lambda T, E, N, D: (T, E, N)),
                 ("terminated_seq", np.uint8, lambda T, E, N, D: (T, E)),
                 ("truncated_seq", np.uint8, lambda T, E, N, D: (T, E)))
ROLLOUT_OUTPUTS = tuple(k for k, _, _ in _ROLLOUT_OUTS)
# ... and of mev_rollout_policy_values, which rollout_policy calls when value_seq is asked for
_VALUE_OUT = ("value_seq", np.float32, lambda T, E, N, D: (T + 1, E, N))
# ... and of mev_rollout_policy_repeat, which it calls with repeat > 1 or when substeps_seq is asked for
_SUBSTEPS_OUT = ("substeps_seq", np.int32, lambda T, E, N, D: (T, E))
_GAE_OUTS = (("advantages", np.float32), ("returns", np.float32), ("valid", np.uint8))


# outputs of evaluate_plans: (key, dtype, shape of (T, C, N))
_EVAL_OUTS = (("returns", np.float32, lambda T, C, N: (C, N)), ("reward_seq", np.float32, lambda T, C, N: (T, C, N)),
              ("done_seq", np.uint8, lambda T, C, N: (T, C, N)), ("status_seq", np.uint8, lambda T, C, N: (T, C, N)),
              ("substeps", np.int32, lambda T, C, N: (C,)), ("terminated", np.uint8, lambda T, C, N: (C,)),
              ("truncated", np.uint8, lambda T, C, N: (C,)))


# (name, dtype, per) — per: "ego" [E*N], "npc" [E*K], "env" [E]; order == struct mev_state
STATE_FIELDS = (
    ("x", np.float32, "ego"), ("y", np.float32, "ego"), ("v", np.float32, "ego"), ("heading", np.float32, "ego"),
    ("acc", np.float32, "ego"), ("steering", np.float32, "ego"), ("prev_dist", np.float32, "ego"),
    ("prev_a0", np.float32, "ego"), ("prev_a1", np.float32, "ego"), ("spawn_x", np.float32, "ego"),
    ("spawn_y", np.float32, "ego"), ("spawn_v", np.float32, "ego"), ("spawn_heading", np.float32, "ego"),
    ("path_index", np.int32, "ego"), ("route", np.int32, "ego"), ("intention", np.int32, "ego"),
    ("alive", np.uint8, "ego"),
    ("npc_x", np.float32, "npc"), ("npc_y", np.float32, "npc"), ("npc_v", np.float32, "npc"),
    ("npc_heading", np.float32, "npc"), ("npc_acc", np.float32, "npc"), ("npc_steering", np.float32, "npc"),
    ("npc_path_index", np.int32, "npc"), ("npc_route", np.int32, "npc"), ("npc_intention", np.int32, "npc"),
    ("npc_alive", np.uint8, "npc"), ("npc_count", np.int32, "env"), ("step_count", np.int32, "env"),
)


class MevState(ctypes.Structure):
    _fields_ = [(name, _vp) for name, _, _ in STATE_FIELDS]


_libs = {}
VARIANT = os.environ.get("MEV_LIB_VARIANT", "")  # "" = product library; "stamps" = diagnostic build


def lib_available() -> bool:
    return os.path.exists(LIB_PATH)


def load_library(variant: str = None):
    """Load libmarlenv_hip.so (building it first when hipcc is present)."""
    variant = VARIANT if variant is None else variant
    if variant in _libs:
        return _libs[variant]
    path = _build.lib_path(variant)
    _one_runtime()
    if not _build.up_to_date(variant) and variant in _build.VARIANTS:  # experiments: tools/variants.py builds them
        try:
            _build.build(variant=variant)
        except Exception as exc:  # no hipcc on this machine: use a prebuilt library if it is there
            if not os.path.exists(path):
                raise RuntimeError(f"{os.path.basename(path)} is missing and could not be built: {exc}") from exc
    L = ctypes.CDLL(path)
    i32p = ctypes.POINTER(ctypes.c_int32)
    f32p = ctypes.POINTER(ctypes.c_float)
    L.mev_last_error.restype = ctypes.c_char_p
    L.mev_config_default.argtypes = [ctypes.POINTER(MevConfig)]
    L.mev_create.argtypes = [ctypes.POINTER(MevConfig), ctypes.POINTER(_vp)]
    L.mev_destroy.argtypes = [_vp]
    L.mev_get_config.argtypes = [_vp, ctypes.POINTER(MevConfig)]
    L.mev_obs_dim.argtypes = [_vp, i32p]
    L.mev_set_stream.argtypes = [_vp, _vp]
    L.mev_sync.argtypes = [_vp]
    L.mev_num_points.argtypes = [_vp, i32p]
    L.mev_point_xy.argtypes = [_vp, ctypes.c_int32, f32p]
    L.mev_route_id.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, i32p]
    L.mev_route_info.argtypes = [_vp, ctypes.c_int32, f32p, i32p, f32p]
    L.mev_set_ego_routes.argtypes = [_vp, i32p]
    L.mev_set_traffic_routes.argtypes = [_vp, i32p, ctypes.c_int32]
    L.mev_default_traffic_routes.argtypes = [_vp, i32p, i32p]
    L.mev_reset.argtypes = [_vp, _vp, _vp, ctypes.c_uint32]
    L.mev_step.argtypes = [_vp, ctypes.POINTER(MevStepArgs)]
    L.mev_step_repeat.argtypes = [_vp, ctypes.POINTER(MevRepeatArgs)]
    L.mev_step_sequence.argtypes = [_vp, ctypes.POINTER(MevSequenceArgs)]
    L.mev_restore_map.argtypes = [_vp, _vp, _vp, ctypes.c_uint32]
    L.mev_evaluate_plans.argtypes = [_vp, ctypes.POINTER(MevEvaluateArgs)]
    L.mev_evaluate_leaves.argtypes = [_vp, ctypes.POINTER(MevLeafArgs)]
    L.mev_pool_create.argtypes = [_vp, ctypes.c_int32, ctypes.POINTER(_vp)]
    L.mev_pool_destroy.argtypes = [_vp]
    L.mev_pool_slots.argtypes = [_vp, i32p]
    L.mev_pool_capture.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_uint32]
    L.mev_pool_get_state.argtypes = [_vp, _vp, ctypes.c_int32, ctypes.POINTER(MevState), _vp, _vp, _vp]
    L.mev_expand_plans.argtypes = [_vp, ctypes.POINTER(MevExpandArgs)]
    L.mev_sample_plans.argtypes = [_vp, ctypes.POINTER(MevSampleArgs)]
    L.mev_sample_expand_plans.argtypes = [_vp, ctypes.POINTER(MevSampleExpandArgs)]
    L.mev_update_plans.argtypes = [_vp, ctypes.POINTER(MevUpdateArgs)]
    L.mev_get_outputs.argtypes = [_vp] + [_vp] * 8 + [ctypes.c_uint32]
    L.mev_get_state.argtypes = [_vp, ctypes.POINTER(MevState)]
    L.mev_set_state.argtypes = [_vp, ctypes.POINTER(MevState)]
    L.mev_device_outputs.argtypes = [_vp] + [ctypes.POINTER(_vp)] * 6
    L.mev_npc_overflow.argtypes = [_vp, ctypes.POINTER(ctypes.c_int64)]
    L.mev_npc_stats.argtypes = [_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.mev_device_count.argtypes = [i32p]
    L.mev_use_own_stream.argtypes = [_vp]
    L.mev_debug_stamps.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64)]
    L.mev_kernel_timing.argtypes = [_vp, ctypes.c_int32]
    L.mev_set_reset_routes.argtypes = [_vp, i32p, ctypes.c_int32]
    L.mev_snapshot_size.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64)]
    L.mev_snapshot.argtypes = [_vp, _vp, ctypes.c_uint32]
    L.mev_restore.argtypes = [_vp, _vp, _vp, ctypes.c_uint32]
    L.mev_kernel_times.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_int64)]
    L.mev_set_step_kernel.argtypes = [_vp, ctypes.c_int32]
    L.mev_get_step_kernel.argtypes = [_vp, i32p]
    L.mev_set_step_pack.argtypes = [_vp, ctypes.c_int32]
    L.mev_get_step_pack.argtypes = [_vp, i32p]
    L.mev_set_step_split.argtypes = [_vp, ctypes.c_int32]
    L.mev_set_env_deal.argtypes = [_vp, ctypes.c_int32]
    L.mev_get_step_split.argtypes = [_vp, i32p]
    L.mev_get_step_row.argtypes = [_vp, i32p, i32p, i32p]
    L.mev_policy_create.argtypes = [_vp, ctypes.POINTER(MevPolicySpec), ctypes.c_uint32, ctypes.POINTER(_vp)]
    L.mev_policy_update.argtypes = [_vp, ctypes.POINTER(MevPolicySpec), ctypes.c_uint32]
    L.mev_policy_destroy.argtypes = [_vp]
    L.mev_rollout_policy.argtypes = [_vp, ctypes.POINTER(MevRolloutArgs)]
    L.mev_get_rollout_row.argtypes = [_vp, i32p]
    L.mev_policy_set_value_head.argtypes = [_vp, _vp, _vp, ctypes.c_uint32]
    L.mev_policy_has_value_head.argtypes = [_vp, i32p]
    L.mev_policy_get_activations.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint32)]
    L.mev_tanh.argtypes = [f32p, f32p, ctypes.c_int64]
    L.mev_rollout_policy_values.argtypes = [_vp, ctypes.POINTER(MevRolloutValuesArgs)]
    L.mev_rollout_policy_repeat.argtypes = [_vp, ctypes.POINTER(MevRolloutRepeatArgs)]
    L.mev_rollout_policies.argtypes = [_vp, ctypes.POINTER(MevRolloutMultiArgs)]
    L.mev_gae.argtypes = [_vp, ctypes.POINTER(MevGaeArgs)]
    L.mev_set_serve.argtypes = [_vp, ctypes.c_int32]
    L.mev_serve_stats.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), i32p]
    L.mev_configure.argtypes = [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.mev_configure_traffic.argtypes = [_vp, ctypes.c_int32, ctypes.c_float]
    L.mev_set_reward.argtypes = [_vp, f32p]
    L.mev_car_update.argtypes = [f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.mev_car_check_collision.argtypes = [f32p, f32p, i32p]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.mev_packed_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, u64p, u64p]
    L.mev_packed_layout2.argtypes = [ctypes.c_int32] * 5 + [u64p, u64p]
    L.mev_set_gather_format.argtypes = [_vp, ctypes.c_int32]
    L.mev_lidar_decode_table.argtypes = [_vp, f32p]
    L.mev_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.mev_comm_init.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.mev_comm_destroy.argtypes = [_vp]
    L.mev_gather_result.argtypes = [_vp, ctypes.POINTER(_vp), u64p, i32p]
    L.mev_gather_wait.argtypes = [_vp, ctypes.c_int32]
    L.mev_unpack_gathered.argtypes = [_vp, _vp, ctypes.c_int32, _vp]
    L.mev_add_route.argtypes = [_vp, f32p, ctypes.c_int32, i32p]
    L.mev_add_route_n.argtypes = [_vp, f32p, ctypes.c_int32, ctypes.c_int32, i32p]
    L.mev_route_len.argtypes = [_vp, ctypes.c_int32, i32p]
    L.mev_output_dlpack.argtypes = [_vp, ctypes.c_int32, ctypes.POINTER(_vp)]
    L.mev_set_car_dims.argtypes = [_vp, f32p, f32p]
    L.mev_get_car_dims.argtypes = [_vp, f32p, f32p]
    L.mev_car_dims_active.argtypes = [_vp, i32p]
    L.mev_set_beam_angles.argtypes = [_vp, f32p]
    L.mev_get_beam_angles.argtypes = [_vp, f32p]
    L.mev_decode_errors.argtypes = [_vp, ctypes.POINTER(ctypes.c_int64)]
    _libs[variant] = L
    return L


class MevError(RuntimeError):
    pass


class IndexRangeError(MevError, IndexError):
    """MEV_E_RANGE: mirrors the reference's std::out_of_range -> IndexError."""


def _check(rc: int):
    if rc != 0:
        msg = load_library().mev_last_error().decode(errors="replace")  # thread-local in the product lib
        if rc == -4:
            raise IndexRangeError(msg)
        raise MevError(f"libmarlenv_hip error {rc}: {msg}")


_OUT_KEYS = ("obs", "reward", "done", "status", "terminated", "truncated", "agents_alive", "step")


class _DLTensor(ctypes.Structure):  # mev_dl_tensor (include/marlenv.h), DLPack's DLTensor
    _fields_ = [("data", ctypes.c_void_p), ("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32),
                ("ndim", ctypes.c_int32), ("dtype_code", ctypes.c_uint8), ("dtype_bits", ctypes.c_uint8),
                ("dtype_lanes", ctypes.c_uint16), ("shape", ctypes.c_void_p), ("strides", ctypes.c_void_p),
                ("byte_offset", ctypes.c_uint64)]


_DL_DELETER = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


class _DLManaged(ctypes.Structure):  # mev_dl_managed, DLPack's DLManagedTensor
    _fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", ctypes.c_void_p), ("deleter", ctypes.c_void_p)]


_DLTENSOR = b"dltensor"


@ctypes.CFUNCTYPE(None, ctypes.c_void_p)
def _capsule_destructor(capsule):
    """PyCapsule destructor: a capsule still named "dltensor" was never consumed (a consumer renames
    it "used_dltensor" and takes over the deleter), so call the managed tensor's deleter."""
    api = ctypes.pythonapi
    api.PyCapsule_IsValid.restype = ctypes.c_int
    api.PyCapsule_IsValid.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    if not api.PyCapsule_IsValid(capsule, _DLTENSOR):
        return
    api.PyCapsule_GetPointer.restype = ctypes.c_void_p
    api.PyCapsule_GetPointer.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    ptr = api.PyCapsule_GetPointer(capsule, _DLTENSOR)
    if ptr:
        m = _DLManaged.from_address(ptr)
        if m.deleter:
            _DL_DELETER(m.deleter)(ptr)


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous, "arrays passed to libmarlenv_hip must be C-contiguous"
        return a.__array_interface__["data"][0]
    if hasattr(a, "data_ptr"):  # torch tensor (device pointer mode)
        return int(a.data_ptr())
    return int(a)


_torch_first_done = False


def _one_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own runtime
    (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7, loaded by path) next to
    the /opt/rocm one this library links by that SONAME.  Imported first, torch's
    copy is already loaded when ours is, and the dynamic linker binds our
    NEEDED libamdhip64.so.7 / librccl.so.1 to it: a single runtime serves both
    (tests/test_capi_symbols.py::test_one_hip_runtime_with_torch).  Loaded the
    other way round, torch would bring its copy in beside ours -- two runtimes in
    one process -- so torch, when installed, is imported before the library.
    MEV_TORCH_FIRST=0 skips this for torch-free processes."""
    if os.environ.get("MEV_TORCH_FIRST", "1") == "0":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _torch_runtime_first():
    """With torch present, let its runtime initialise the device before the
    library's first HIP call (the same single runtime, see _one_runtime).
    Set MEV_TORCH_FIRST=0 for torch-free processes."""
    global _torch_first_done
    if _torch_first_done:
        return
    _torch_first_done = True
    if os.environ.get("MEV_TORCH_FIRST", "1") == "0":
        return
    try:
        import torch
    except ImportError:
        return
    try:
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


def default_config() -> Dict:
    c = MevConfig()
    _check(load_library().mev_config_default(ctypes.byref(c)))
    d = {name: getattr(c, name) for name, _ in MevConfig._fields_}
    d["reward"] = list(c.reward)
    return d


class Handle:
    """One device-resident batch of E intersection envs (owner of a mev_handle)."""

    def __init__(self, **cfg):
        _torch_runtime_first()
        L = load_library()
        c = MevConfig()
        _check(L.mev_config_default(ctypes.byref(c)))
        for k, v in cfg.items():
            if k == "reward":
                for j, x in enumerate(v):
                    c.reward[j] = float(x)
            elif not hasattr(c, k):
                raise TypeError(f"unknown config key {k!r}")
            else:
                setattr(c, k, v)
        h = _vp()
        _check(L.mev_create(ctypes.byref(c), ctypes.byref(h)))
        self._args_cache = None
        self._h = h
        self._lib = L
        out = MevConfig()
        _check(L.mev_get_config(h, ctypes.byref(out)))
        self.config = {name: getattr(out, name) for name, _ in MevConfig._fields_}
        self.config["reward"] = list(out.reward)
        self.E = out.num_envs
        self.N = out.num_agents
        self.K = out.max_npcs
        self.R = out.lidar_rays
        self.D = out.obs_dim
        n = ctypes.c_int32()
        _check(L.mev_num_points(h, ctypes.byref(n)))
        self.num_points = n.value

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.mev_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: Optional[int]):
        """Order this handle's work on a hipStream_t (int handle; 0/None = legacy default stream)."""
        _check(self._lib.mev_set_stream(self._h, stream_ptr or None))

    def use_own_stream(self):
        _check(self._lib.mev_use_own_stream(self._h))

    def debug_stamps(self) -> np.ndarray:
        out = np.zeros((self.E, 8), np.uint64)
        _check(self._lib.mev_debug_stamps(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def sync(self):
        _check(self._lib.mev_sync(self._h))

    # -- routes -----------------------------------------------------------
    def route_id(self, start_point: int, end_point: int) -> int:
        r = ctypes.c_int32()
        _check(self._lib.mev_route_id(self._h, int(start_point), int(end_point), ctypes.byref(r)))
        return r.value

    def route_info(self, route: int):
        """(path [max(n, 160), 2] -- a shorter path padded with its last point --, intent, spawn)."""
        path = np.zeros((max(PATH_LEN, self.route_len(route)), 2), np.float32)
        intent = ctypes.c_int32()
        spawn = np.zeros(3, np.float32)
        _check(self._lib.mev_route_info(self._h, int(route), path.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                        ctypes.byref(intent), spawn.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return path, intent.value, spawn

    def route_len(self, route: int) -> int:
        """Points of a route's path (160, or a written path's own n; mev_route_len)."""
        n = ctypes.c_int32()
        _check(self._lib.mev_route_len(self._h, int(route), ctypes.byref(n)))
        return n.value

    def add_route(self, path, intent: int) -> int:
        """Append a route of the caller's own (path [n, 2] f32 with 2 <= n <= 4096, intent 0 straight /
        1 left / 2 right) to the route table (mev_add_route_n); returns its id."""
        a = np.ascontiguousarray(path, np.float32)
        if a.ndim != 2 or a.shape[1] != 2 or not 2 <= a.shape[0] <= MAX_PATH_LEN:
            raise ValueError(f"a route path has 2 .. {MAX_PATH_LEN} points (x, y), got shape {a.shape}")
        r = ctypes.c_int32()
        _check(self._lib.mev_add_route_n(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.shape[0],
                                         int(intent), ctypes.byref(r)))
        return r.value

    def point_xy(self, point: int):
        xy = np.zeros(2, np.float32)
        _check(self._lib.mev_point_xy(self._h, int(point), xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return xy

    def set_ego_routes(self, routes):
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(routes, np.int32), (self.E, self.N)), np.int32)
        _check(self._lib.mev_set_ego_routes(self._h, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))

    def set_traffic_routes(self, routes):
        r = np.ascontiguousarray(np.asarray(routes, np.int32).reshape(-1))
        _check(self._lib.mev_set_traffic_routes(self._h, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(r)))

    def default_traffic_routes(self):
        cnt = ctypes.c_int32()
        buf = np.zeros(1024, np.int32)
        _check(self._lib.mev_default_traffic_routes(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                    ctypes.byref(cnt)))
        return buf[: cnt.value].copy()

    # -- reset / step -----------------------------------------------------
    def reset(self, env_mask=None, obs=None, device: bool = False):
        mask = None if env_mask is None else (env_mask if device else np.ascontiguousarray(env_mask, np.uint8))
        _check(self._lib.mev_reset(self._h, _ptr(mask), _ptr(obs), MEV_DEVICE_PTRS if device else 0))
        return obs

    def alloc_outputs(self):
        E, N, D = self.E, self.N, self.D
        return dict(obs=np.zeros((E, N, D), np.float32), reward=np.zeros((E, N), np.float32),
                    done=np.zeros((E, N), np.uint8), status=np.zeros((E, N), np.uint8),
                    terminated=np.zeros(E, np.uint8), truncated=np.zeros(E, np.uint8),
                    agents_alive=np.zeros(E, np.int32), step=np.zeros(E, np.int32))

    def step(self, actions, dt: float = 1.0 / 60.0, out: Optional[dict] = None, spawn_route=None,
             auto_reset: bool = False, device: bool = False, gather: bool = False):
        """Host mode (default): numpy in/out, synchronous.  device=True: every
        array is a device tensor/pointer on this handle's device; asynchronous.
        gather=True (needs comm_init): the outputs are written packed and
        gathered to the root rank over RCCL (gather_result); `out` may then
        only hold agents_alive / step."""
        if not device:
            actions = np.ascontiguousarray(actions, np.float32)
            if actions.size != self.E * self.N * 2:
                raise ValueError(f"actions must have {self.E}x{self.N}x2 elements, got {actions.shape}")
            if spawn_route is not None:
                spawn_route = np.ascontiguousarray(np.broadcast_to(np.asarray(spawn_route, np.int32), (self.E,)))
            if out is None and not gather:
                out = self.alloc_outputs()
        out = out or {}
        # the output pointers of the args struct are reused while `out` holds the same
        # arrays (a step loop passes one dict): numpy pointer lookups cost ~1.6 us each
        c = self._args_cache
        if c is None or c[0] is not out or not all(map(operator.is_, c[1], map(out.get, _OUT_KEYS))):
            a = MevStepArgs()
            for k in _OUT_KEYS:
                setattr(a, k, _ptr(out.get(k)))
            c = self._args_cache = (out, tuple(map(out.get, _OUT_KEYS)), a, None)
        a = c[2]
        if actions is not c[3]:  # (a loop that refills one actions array skips the pointer lookup)
            a.actions = _ptr(actions)
            c = self._args_cache = (c[0], c[1], a, actions)
        a.dt = float(dt)
        a.spawn_route = _ptr(spawn_route)
        a.flags = ((MEV_DEVICE_PTRS if device else 0) | (MEV_AUTO_RESET if auto_reset else 0) |
                   (MEV_GATHER_TO_ROOT if gather else 0))
        _check(self._lib.mev_step(self._h, ctypes.byref(a)))
        return out

    def step_repeat(self, actions, repeat: int, dt: float = 1.0 / 60.0, out: Optional[dict] = None, spawn_route=None,
                    auto_reset: bool = False, device: bool = False, gather: bool = False):
        """Frame skip (mev_step_repeat): hold `actions` for up to `repeat` sub-steps of every env
        in one call -- the reward summed, done / status latched, each env stopping at its first
        terminated or truncated sub-step -- and cast the LiDAR once, from the state it stopped
        at.  Returns the outputs of `step` plus `substeps` [E] (sub-steps executed).
        spawn_route, if given, is [repeat][E].  device=True: every array (a `substeps` entry of
        `out` included) is a device tensor/pointer.  gather: not supported (the library rejects it)."""
        if not device:
            actions, spawn_route, out = self._window_host(actions, False, int(repeat), spawn_route, out)
        out = out if out is not None else {}
        a = MevRepeatArgs()
        self._fill_step_args(a.step, out, actions, spawn_route, auto_reset, device, gather)
        a.step.dt = float(dt)
        a.repeat = int(repeat)
        a.substeps = _ptr(out.get("substeps"))
        _check(self._lib.mev_step_repeat(self._h, ctypes.byref(a)))
        return out

    def _window_host(self, actions, plan, n, spawn_route, out):
        """Host mode of a window of n sub-steps (step_repeat, step_sequence): actions as float32,
        one held [E][N][2] row or (plan) n rows; spawn_route as [n][E] int32; `out` with the
        outputs of `step` and `substeps`."""
        actions = np.ascontiguousarray(actions, np.float32)
        if plan and (actions.ndim < 2 or actions.size != n * self.E * self.N * 2):
            raise ValueError(f"actions must be [T][{self.E}][{self.N}][2], got {actions.shape}")
        if not plan and actions.size != self.E * self.N * 2:
            raise ValueError(f"actions must have {self.E}x{self.N}x2 elements, got {actions.shape}")
        if spawn_route is not None:
            spawn_route = np.ascontiguousarray(np.asarray(spawn_route, np.int32))
            if spawn_route.shape != (n, self.E):
                raise ValueError(f"spawn_route must be [{n}][{self.E}], got {spawn_route.shape}")
        if out is None:
            out = self.alloc_outputs()
        if out.get("substeps") is None:
            out["substeps"] = np.zeros(self.E, np.int32)
        return actions, spawn_route, out

    @staticmethod
    def _fill_step_args(a, out, actions, spawn_route, auto_reset, device, gather):
        for k in _OUT_KEYS:
            setattr(a, k, _ptr(out.get(k)))
        a.actions = _ptr(actions)
        a.spawn_route = _ptr(spawn_route)
        a.flags = ((MEV_DEVICE_PTRS if device else 0) | (MEV_AUTO_RESET if auto_reset else 0) |
                   (MEV_GATHER_TO_ROOT if gather else 0))

    def step_sequence(self, actions, dt=1.0 / 60.0, out: Optional[dict] = None, spawn_route=None,
                      auto_reset: bool = False, device: bool = False, gather: bool = False, length: Optional[int] = None):
        """Open-loop plan rollout (mev_step_sequence): actions [T][E][N][2], row s the action of
        sub-step s + 1; dt a float or a sequence of T floats (always host values).  Each env
        stops at its first terminated or truncated sub-step; the LiDAR is cast once, from the
        state it stopped at.  Returns the outputs of `step` (reward summed, done / status latched,
        as `step_repeat`) plus `substeps` [E] and `reward_seq`, `done_seq`, `status_seq`
        [T][E][N]: each executed sub-step's own outputs, zero after an env stopped.
        spawn_route, if given, is [T][E].  device=True: every array (the `substeps` / `*_seq`
        entries of `out` included; absent ones are not written) is a device tensor/pointer and T
        is actions.shape[0] (or `length` for a raw pointer).  gather: not supported."""
        if length is None:
            shape = getattr(actions, "shape", None) if device else np.shape(actions)
            if not shape:
                raise ValueError("step_sequence needs actions of shape [T][E][N][2] (or length=T)")
            length = int(shape[0])
        T = int(length)
        if not device:
            actions, spawn_route, out = self._window_host(actions, True, T, spawn_route, out)
            for k, dtype in zip(_SEQ_KEYS, (np.float32, np.uint8, np.uint8)):
                if out.get(k) is None or out[k].shape != (T, self.E, self.N):
                    out[k] = np.zeros((T, self.E, self.N), dtype)
        out = out if out is not None else {}
        a = MevSequenceArgs()
        self._fill_step_args(a.step, out, actions, spawn_route, auto_reset, device, gather)
        a.length = T
        dts = None
        if np.ndim(dt) == 0:
            a.step.dt = float(dt)
        else:
            dts = np.ascontiguousarray(dt, np.float32).reshape(-1)
            if dts.size != T:
                raise ValueError(f"dt must be a float or {T} floats, got {dts.size}")
            a.step.dt = float(dts[0]) if T else 0.0
            a.dt_seq = dts.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        for k in _SEQ_KEYS:
            setattr(a, k, _ptr(out.get(k)))
        a.substeps = _ptr(out.get("substeps"))
        _check(self._lib.mev_step_sequence(self._h, ctypes.byref(a)))
        return out

    def _plan_args(self, a, need, lead, roots, rl, per, count, length, dt, gamma, spawn_route, out, device, flags,
                   leaf_obs, extra=()):
        """The part every plan call shares, filled into `a` (a MevEvaluateArgs; `actions` is the
        caller's): roots [R] with R = `count` or roots.shape[0] (`rl`: R's letter in the messages), C =
        R * per candidates, T = `length` or lead.shape[0] (`lead`: the caller's actions or mean; `need`:
        the message when device mode cannot tell T or R), spawn_route [T][C], dt and the outputs --
        _EVAL_OUTS, `extra` in the same form, leaf_obs if asked for; host mode creates what an empty
        `out` lacks and checks shapes and dtypes.  Returns T, C, R, out and the arrays `a` points into,
        which the caller holds until the C call has returned."""
        N = self.N
        if device:
            if length is None:
                length = getattr(lead, "shape", (None,))[0]
            if count is None:
                count = getattr(roots, "shape", (None,))[0]
            if length is None or count is None:
                raise ValueError(need)
            T, R = int(length), int(count)
            C = R * per
            out = out if out is not None else {}
        else:
            roots = np.ascontiguousarray(roots, np.int32)
            if roots.ndim != 1:
                raise ValueError(f"roots must be [{rl}], got {roots.shape}")
            R = int(roots.shape[0]) if count is None else int(count)
            T = (int(lead.shape[0]) if lead.ndim else 0) if length is None else int(length)
            C = R * per
            if roots.shape != (R,):
                raise ValueError(f"roots must be [{R}], got {roots.shape}")
            if spawn_route is not None:
                spawn_route = np.ascontiguousarray(np.asarray(spawn_route, np.int32))
                if spawn_route.shape != (T, C):
                    raise ValueError(f"spawn_route must be [{T}][{C}], got {spawn_route.shape}")
            out = out if out is not None else {}
            outs = _EVAL_OUTS + tuple(extra)
            if not out:
                for k, dtype, shape in outs:
                    out[k] = np.zeros(shape(T, C, N), dtype)
            if leaf_obs:
                if out.get("leaf_obs") is None:
                    out["leaf_obs"] = np.zeros((C, N, self.D), np.float32)
                outs += (("leaf_obs", np.float32, lambda T, C, N: (C, N, self.D)),)
            for k, dtype, shape in outs:
                if out.get(k) is not None and (out[k].shape != shape(T, C, N) or out[k].dtype != dtype):
                    raise ValueError(f"{k} must be {np.dtype(dtype).name} {list(shape(T, C, N))}, got {out[k].shape}")
        a.roots, a.spawn_route = _ptr(roots), _ptr(spawn_route)
        a.candidates, a.length, a.gamma = C, T, float(gamma)
        dts = None
        if np.ndim(dt) == 0:
            a.dt = float(dt)
        else:
            dts = np.ascontiguousarray(dt, np.float32).reshape(-1)
            if dts.size != T:
                raise ValueError(f"dt must be a float or {T} floats, got {dts.size}")
            a.dt = float(dts[0]) if T else 0.0
            a.dt_seq = dts.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        for k, _, _ in _EVAL_OUTS:
            setattr(a, k, _ptr(out.get(k)))
        a.flags = (MEV_DEVICE_PTRS if device else 0) | int(flags)
        return T, C, R, out, (roots, spawn_route, dts)

    def evaluate_plans(self, actions, roots, dt=1.0 / 60.0, gamma: float = 1.0, spawn_route=None,
                       out: Optional[dict] = None, device: bool = False, candidates: Optional[int] = None,
                       length: Optional[int] = None, flags: int = 0, leaf_obs: bool = False, _expand=None):
        """Score candidate plans from the live batch (mev_evaluate_plans); the handle stays as it is.
        actions [T][C][N][2], roots [C] (the live env each candidate starts from), dt a float or T
        floats (always host values), spawn_route optional [T][C].  Returns `returns` [C][N] (the
        discounted f32 return), `reward_seq`, `done_seq`, `status_seq` [T][C][N] (zero after a
        candidate stopped), `substeps`, `terminated`, `truncated` [C].  No observation, no LiDAR.
        device=True: every array is a device tensor/pointer, only the outputs present in `out` are
        written, and C, T are roots.shape[0], actions.shape[0] (or `candidates` / `length` for raw
        pointers).  flags: further bits for the call's flags word (the library refuses them).
        leaf_obs=True (mev_evaluate_leaves): the result gains `leaf_obs` [C][N][obs_dim], the
        observation of the state each candidate stopped at (head and LiDAR block; every float
        written).  In device mode out["leaf_obs"] must be there; the other outputs are optional."""
        if not device:
            actions = np.ascontiguousarray(actions, np.float32)
        la = MevLeafArgs()
        a = la.eval
        T, C, _, out, _keep = self._plan_args(
            a, "evaluate_plans needs actions [T][C][N][2] and roots [C] (or length=T, candidates=C)", actions, roots,
            "C", 1, candidates, length, dt, gamma, spawn_route, out, device, flags, leaf_obs)
        if not device and actions.shape != (T, C, self.N, 2):
            raise ValueError(f"actions must be [{T}][{C}][{self.N}][2], got {actions.shape}")
        a.actions = _ptr(actions)
        if _expand is not None:
            xa = MevExpandArgs()
            xa.eval = a
            xa.leaf_obs = _ptr(out.get("leaf_obs")) if leaf_obs else None
            xa.src, xa.dst, xa.dst_slots, xa.counter_offset = _expand
            _check(self._lib.mev_expand_plans(self._h, ctypes.byref(xa)))
        elif leaf_obs:
            la.leaf_obs = _ptr(out.get("leaf_obs"))
            _check(self._lib.mev_evaluate_leaves(self._h, ctypes.byref(la)))
        else:
            _check(self._lib.mev_evaluate_plans(self._h, ctypes.byref(a)))
        return out

    def pool(self, slots: int) -> "Pool":
        """A state pool of `slots` slots (mev_pool_create): env states kept on the device outside the
        live batch, filled by Pool.capture and expand_plans, read by expand_plans(src=pool)."""
        return Pool(self, slots)

    def expand_plans(self, actions, roots, dst: "Pool", dst_slots, src: Optional["Pool"] = None,
                     counter_offset: int = 0, leaf_obs: bool = False, dt=1.0 / 60.0, gamma: float = 1.0,
                     spawn_route=None, out: Optional[dict] = None, device: bool = False,
                     candidates: Optional[int] = None, length: Optional[int] = None, flags: int = 0):
        """evaluate_plans (leaf_obs=True: with the leaf observations) whose candidates start from the
        slots roots[c] of pool `src` (None: from live envs) and whose stop states are stored in the
        slots dst_slots[c] of pool `dst` (-1: not stored) -- mev_expand_plans.  The Philox spawner of
        sub-step s uses the handle's counter + counter_offset + (s - 1).  Everything else follows
        evaluate_plans' conventions; in device mode dst_slots is a device array like roots, and an
        empty `out` is allowed (the pool is an output)."""
        if not device:
            dst_slots = np.ascontiguousarray(dst_slots, np.int32)
            if dst_slots.shape != np.shape(roots):
                raise ValueError(f"dst_slots must have roots' shape {np.shape(roots)}, got {dst_slots.shape}")
        xp = (src._p if src is not None else None, dst._p if dst is not None else None, _ptr(dst_slots),
              int(counter_offset))
        return self.evaluate_plans(actions, roots, dt, gamma, spawn_route, out, device, candidates, length, flags,
                                   leaf_obs, _expand=xp)

    def sample_plans(self, mean, sigma, roots, samples: int, dt=1.0 / 60.0, gamma: float = 1.0, lo=(-1.0, -1.0),
                     hi=(1.0, 1.0), seed: int = 0, counter: int = 0, mean_first: bool = False, leaf_obs: bool = False,
                     spawn_route=None, out: Optional[dict] = None, device: bool = False, groups: Optional[int] = None,
                     length: Optional[int] = None, flags: int = 0, sample_flags: Optional[int] = None,
                     src: Optional["Pool"] = None, dst: Optional["Pool"] = None, dst_slots=None,
                     counter_offset: int = 0):
        """evaluate_plans (leaf_obs=True: with the leaf observations) whose candidates draw their own
        actions on the device -- mev_sample_plans.  mean, sigma [T][G][N][2], roots [G] (the live env
        of each group); candidate c = g * samples + j runs clamp(mean + sigma * eps, lo, hi) with eps
        the Irwin-Hall approximation of a unit Gaussian that include/marlenv.h states, from the
        Philox stream (seed, counter).  mean_first: candidate j == 0 of every group runs the clamped
        mean.  Returns evaluate_plans' outputs over C = G * samples candidates plus `actions_out`
        [T][C][N][2], the actions the candidates ran (every element written).  device=True: every
        array is a device tensor/pointer and only the outputs present in `out` are written; T and G
        are mean.shape[0] and roots.shape[0] (or `length` / `groups` for raw pointers).
        dst (mev_sample_expand_plans): the candidates' stop states go to the slots dst_slots[c] ([C];
        -1: not stored) of pool `dst`, the groups start from the slots roots[g] of pool `src` (None:
        from live envs), and the Philox spawner of sub-step s uses the handle's counter +
        counter_offset + (s - 1), all as expand_plans defines them; an empty `out` is allowed in
        device mode (the pool is an output).  src or dst_slots without dst: ValueError."""
        N, K = self.N, int(samples)
        if dst is None and (src is not None or dst_slots is not None):
            raise ValueError("src and dst_slots need dst (the pool that receives the stop states)")
        if not device:
            mean = np.ascontiguousarray(mean, np.float32)
            sigma = np.ascontiguousarray(sigma, np.float32)
        xa = MevSampleExpandArgs()
        sa = xa.sample
        T, C, G, out, _keep = self._plan_args(
            sa.eval, "sample_plans needs mean [T][G][N][2] and roots [G] (or length=T, groups=G)", mean, roots, "G", K,
            groups, length, dt, gamma, spawn_route, out, device, flags, leaf_obs,
            extra=(("actions_out", np.float32, lambda T, C, N: (T, C, N, 2)),))
        if not device and (mean.shape != (T, G, N, 2) or sigma.shape != mean.shape):
            raise ValueError(f"mean and sigma must be [{T}][{G}][{N}][2], got {mean.shape} and {sigma.shape}")
        sa.leaf_obs = _ptr(out.get("leaf_obs")) if leaf_obs else None
        sa.mean, sa.sigma, sa.actions_out = _ptr(mean), _ptr(sigma), _ptr(out.get("actions_out"))
        sa.lo = (ctypes.c_float * 2)(*[float(v) for v in lo])
        sa.hi = (ctypes.c_float * 2)(*[float(v) for v in hi])
        sa.groups, sa.samples = G, K
        sa.noise_seed, sa.noise_counter = int(seed) & (2**64 - 1), int(counter) & (2**64 - 1)
        sa.sample_flags = (MEV_SAMPLE_MEAN_FIRST if mean_first else 0) if sample_flags is None else int(sample_flags)
        if dst is None:
            _check(self._lib.mev_sample_plans(self._h, ctypes.byref(sa)))
            return out
        if not device and dst_slots is not None:
            dst_slots = np.ascontiguousarray(dst_slots, np.int32)
            if dst_slots.shape != (C,):
                raise ValueError(f"dst_slots must be [{C}], got {dst_slots.shape}")
        xa.src, xa.dst, xa.dst_slots = src._p if src is not None else None, dst._p, _ptr(dst_slots)
        xa.counter_offset = int(counter_offset)
        _check(self._lib.mev_sample_expand_plans(self._h, ctypes.byref(xa)))
        return out

    def policy(self, weights, biases, device: bool = False, hidden: str = "relu", out: str = "linear") -> "Policy":
        """An MLP policy held by the library (mev_policy_create): weights a list of 2 or 3 arrays [out][in]
        (torch.nn.Linear.weight's layout; the first takes obs_dim inputs, the last has 2 outputs), biases
        the matching [out] arrays.  device=True: device tensors / pointers (then no check, no sync).
        hidden: "relu" or "tanh", the activation of every hidden layer; out: "linear" or "tanh", the latter
        squashing mu before noise and clamp (tanh_c, the library's stated f32 tanh).  Fixed at creation."""
        return Policy(self, weights, biases, device, hidden=hidden, out=out)

    def rollout_row(self) -> int:
        """The row of k_rollout's table rollout_policy runs for this handle (mev_get_rollout_row); -1: unsupported."""
        r = ctypes.c_int32()
        _check(self._lib.mev_get_rollout_row(self._h, ctypes.byref(r)))
        return r.value

    def rollout_policy(self, policy: "Policy", T: int, dt: float = 1.0 / 60.0, sigma=None, lo=(-1.0, -1.0),
                       hi=(1.0, 1.0), seed: int = 0, counter: int = 0, auto_reset: bool = False, spawn_route=None,
                       outputs=ROLLOUT_OUTPUTS, out: Optional[dict] = None, device: bool = False, flags: int = 0,
                       repeat: int = 1, _multi=None):
        """Closed-loop rollout (mev_rollout_policy): T sub-steps of observe -> policy -> step in one launch,
        bit for bit the loop of the stated policy arithmetic and `step`.  sigma: None (deterministic) or
        two host floats; the noise is sample_plans' from the Philox stream (seed, counter) with the env in
        the candidate's place.  spawn_route optional [T][E].  Returns a dict with the arrays named in
        `outputs` (ROLLOUT_OUTPUTS: obs_seq [T][E][N][obs_dim], actions_seq / mean_seq [T][E][N][2],
        reward_seq / done_seq / status_seq [T][E][N], terminated_seq / truncated_seq [T][E]); `out` may
        hold preallocated ones.  device=True: device tensors, stream-ordered, no host sync -- the arrays
        of `out`, or new torch tensors for `outputs`; spawn_route is then a device array too.
        With "value_seq" among the outputs (or in `out`) the call is mev_rollout_policy_values: the policy
        needs a value head (Policy.set_value_head) and value_seq [T + 1][E][N] holds V(obs_t), row T the
        bootstrap value; everything else is the same bits.
        repeat > 1, or "substeps_seq" among the outputs, makes the call mev_rollout_policy_repeat: T DECISIONS,
        each one policy pass and then `step_repeat` with that action held for up to `repeat` sub-steps -- every
        *_seq row is then a decision's (summed reward, latched done / status, one LiDAR cast), the noise word
        index is the decision, spawn_route is [T][repeat][E], T * repeat <= MEV_MAX_ROLLOUT_SUBSTEPS, and
        substeps_seq [T][E] (int32) holds the sub-steps each decision ran.  With repeat = 1 the outputs are
        those of the other two calls bit for bit."""
        T, E, N, D, repeat = int(T), self.E, self.N, self.D, int(repeat)
        shapes = {k: (dtype, shape(T, E, N, D)) for k, dtype, shape in _ROLLOUT_OUTS + (_VALUE_OUT, _SUBSTEPS_OUT)}
        named = outputs if out is None or not out else out
        values = "value_seq" in named
        held = repeat != 1 or "substeps_seq" in named  # (today's calls take today's path)
        held = held or _multi is not None  # (rollout_policies: the frame-skip call's arguments)
        out = dict(out) if out is not None else {}
        for k in out:
            if k not in shapes:
                raise ValueError(f"unknown rollout output {k!r}")
        if device:
            missing = [k for k in outputs if out.get(k) is None] if not out else []
            if missing:
                import torch
                dev = f"cuda:{self.config['device']}"
                for k in missing:
                    dtype, shape = shapes[k]
                    tdt = torch.float32 if dtype is np.float32 else torch.int32 if dtype is np.int32 else torch.uint8
                    out[k] = torch.empty(shape, dtype=tdt, device=dev)
        else:
            if spawn_route is not None:
                spawn_route = np.ascontiguousarray(np.asarray(spawn_route, np.int32))
                want = (T, repeat, E) if held else (T, E)
                if spawn_route.shape != want and not (held and repeat == 1 and spawn_route.shape == (T, E)):
                    raise ValueError(f"spawn_route must be {list(want)}, got {spawn_route.shape}")
            if not out:
                for k in outputs:
                    out[k] = np.zeros(shapes[k][1], shapes[k][0])
            for k, v in out.items():
                if v is not None and (v.shape != shapes[k][1] or v.dtype != shapes[k][0]):
                    raise ValueError(f"{k} must be {np.dtype(shapes[k][0]).name} {list(shapes[k][1])}, got {v.shape}")
        a = MevRolloutArgs()
        a.policy = policy._p if policy is not None else None
        a.length, a.dt = T, float(dt)
        a.spawn_route = _ptr(spawn_route)
        sig = None
        if sigma is not None:
            sig = (ctypes.c_float * 2)(*[float(v) for v in sigma])
            a.sigma = ctypes.cast(sig, ctypes.POINTER(ctypes.c_float))
        a.lo = (ctypes.c_float * 2)(*[float(v) for v in lo])
        a.hi = (ctypes.c_float * 2)(*[float(v) for v in hi])
        a.noise_seed, a.noise_counter = int(seed) & (2**64 - 1), int(counter) & (2**64 - 1)
        for k in ROLLOUT_OUTPUTS:
            setattr(a, k, _ptr(out.get(k)))
        a.flags = (MEV_DEVICE_PTRS if device else 0) | (MEV_AUTO_RESET if auto_reset else 0) | int(flags)
        if held:
            ra = MevRolloutRepeatArgs()
            ra.rollout, ra.value_seq, ra.repeat = a, _ptr(out.get("value_seq")), repeat
            ra.substeps_seq = _ptr(out.get("substeps_seq"))
            if values and ra.value_seq is None:
                raise ValueError("value_seq is named but not given")
            if _multi is not None:
                ma = MevRolloutMultiArgs()
                ma.base, (ma.policies, ma.count, ma.assign, ma.sigma) = ra, _multi
                _check(self._lib.mev_rollout_policies(self._h, ctypes.byref(ma)))
            else:
                _check(self._lib.mev_rollout_policy_repeat(self._h, ctypes.byref(ra)))
        elif values:
            va = MevRolloutValuesArgs()
            va.rollout, va.value_seq = a, _ptr(out.get("value_seq"))
            _check(self._lib.mev_rollout_policy_values(self._h, ctypes.byref(va)))
        else:
            _check(self._lib.mev_rollout_policy(self._h, ctypes.byref(a)))
        return out

    def rollout_policies(self, policies, assign, T: int, dt: float = 1.0 / 60.0, sigma=None, lo=(-1.0, -1.0),
                         hi=(1.0, 1.0), seed: int = 0, counter: int = 0, auto_reset: bool = False, spawn_route=None,
                         outputs=ROLLOUT_OUTPUTS, out: Optional[dict] = None, device: bool = False, flags: int = 0,
                         repeat: int = 1):
        """A policy per agent slot in one rollout (mev_rollout_policies): rollout_policy(..., repeat=repeat) with
        agent slot (e, i) driven by policies[assign[e][i]] for the whole call -- that policy's own layers, sigma row
        and value head; the noise word does not depend on the policy.  policies: 1..MEV_MAX_ROLLOUT_POLICIES Policy
        objects of this handle (depths and widths may differ); assign: uint8 [E][N] (a device tensor with
        device=True, where an entry >= len(policies) is read as the last policy; on the host it raises
        IndexRangeError); sigma: None or host floats [P][2].  Returns the same dict as rollout_policy; "value_seq"
        (every listed policy then needs a value head) and "substeps_seq" are available the same way.  One policy
        and assign all zero give rollout_policy's bits."""
        policies = list(policies) if policies is not None else None
        count = len(policies) if policies is not None else 0
        table = None
        if policies is not None:
            table = (_vp * max(count, 1))(*[p._p if p is not None else None for p in policies])
        if not device and assign is not None:
            assign = np.ascontiguousarray(assign)
            if assign.dtype != np.uint8 or assign.shape != (self.E, self.N):
                raise ValueError(f"assign must be uint8 {[self.E, self.N]}, got {assign.dtype} {list(assign.shape)}")
        sig = None
        if sigma is not None:
            flat = np.asarray(sigma, np.float32).reshape(-1)
            if flat.size != 2 * count:
                raise ValueError(f"sigma must be [{count}][2]")
            sig = (ctypes.c_float * max(flat.size, 1))(*flat.tolist())
        multi = (ctypes.cast(table, ctypes.POINTER(_vp)) if table is not None else None, count, _ptr(assign),
                 ctypes.cast(sig, ctypes.POINTER(ctypes.c_float)) if sig is not None else None)
        return self.rollout_policy(None, T, dt=dt, sigma=None, lo=lo, hi=hi, seed=seed, counter=counter,
                                   auto_reset=auto_reset, spawn_route=spawn_route, outputs=outputs, out=out,
                                   device=device, flags=flags, repeat=repeat, _multi=multi)

    def gae(self, reward_seq, value_seq, done_seq=None, terminated_seq=None, truncated_seq=None, ended_before=None,
            gamma: float = 0.99, lam: float = 0.95, mask_reset_steps: bool = False,
            outputs=("advantages", "returns"), out: Optional[dict] = None, device: bool = False, flags: int = 0):
        """Generalised advantage estimation (mev_gae) over a rollout's arrays: reward_seq [T][E][N], value_seq
        [T + 1][E][N], optional done_seq [T][E][N], terminated_seq / truncated_seq [T][E], ended_before [E].
        An agent's done or the env's termination stops the bootstrap and the trace, a truncation bootstraps
        and cuts the trace; mask_reset_steps zeroes the transitions that follow an env's end (the auto-reset
        steps) and clears their `valid`.  Returns the arrays named in `outputs` ("advantages", "returns",
        "valid", each [T][E][N]); `out` may hold preallocated ones.  device=True: device tensors,
        stream-ordered, no host sync."""
        E, N = self.E, self.N
        names = {k: dtype for k, dtype in _GAE_OUTS}
        out = dict(out) if out is not None else {}
        for k in list(out) + (list(outputs) if not out else []):
            if k not in names:
                raise ValueError(f"unknown gae output {k!r}")
        ins = dict(reward_seq=reward_seq, value_seq=value_seq, done_seq=done_seq, terminated_seq=terminated_seq,
                   truncated_seq=truncated_seq, ended_before=ended_before)
        if device:
            T = int(reward_seq.shape[0])
            if not out:
                import torch
                for k in outputs:
                    out[k] = torch.empty((T, E, N), dtype=torch.float32 if names[k] is np.float32 else torch.uint8,
                                         device=f"cuda:{self.config['device']}")
        else:
            reward_seq = np.asarray(reward_seq)
            T = int(reward_seq.shape[0]) if reward_seq.ndim == 3 else 0
            want = dict(reward_seq=((T, E, N), np.float32), value_seq=((T + 1, E, N), np.float32),
                        done_seq=((T, E, N), np.uint8), terminated_seq=((T, E), np.uint8),
                        truncated_seq=((T, E), np.uint8), ended_before=((E,), np.uint8))
            for k, (shape, dtype) in want.items():
                if ins[k] is None:
                    continue
                v = np.asarray(ins[k])
                if v.dtype == np.bool_:
                    v = v.astype(np.uint8)
                ins[k] = np.ascontiguousarray(v, dtype)
                if ins[k].shape != shape:
                    raise ValueError(f"{k} must be {list(shape)}, got {ins[k].shape}")
            if not out:
                for k in outputs:
                    out[k] = np.zeros((T, E, N), names[k])
            for k, v in out.items():
                if v is not None and (v.shape != (T, E, N) or v.dtype != names[k]):
                    raise ValueError(f"{k} must be {np.dtype(names[k]).name} {[T, E, N]}, got {v.shape}")
        ga = MevGaeArgs()
        for k, v in ins.items():
            setattr(ga, k, _ptr(v))
        ga.length, ga.gamma, ga.lam = T, float(gamma), float(lam)
        for k in names:
            setattr(ga, k, _ptr(out.get(k)))
        ga.flags = (MEV_DEVICE_PTRS if device else 0) | (MEV_GAE_MASK_RESET_STEPS if mask_reset_steps else 0) | int(flags)
        _check(self._lib.mev_gae(self._h, ctypes.byref(ga)))
        return out

    def update_plans(self, actions, samples: int, scores=None, returns=None, mode: str = "elites",
                     elites: Optional[int] = None, temperature: float = 1.0, sigma_min: float = 0.0,
                     out: Optional[dict] = None, device: bool = False, groups: Optional[int] = None,
                     length: Optional[int] = None, flags: int = 0):
        """Rank each group's `samples` candidates and refit mean and sigma -- mev_update_plans.
        actions [T][C][N][2] (C = G * samples), the score of candidate c is scores[c] or the f32 sum
        of returns[c].  mode "elites": the `elites` best, exact; "softmax": weights
        exp((score - best) / temperature) (temperature = inf: equal weights).  Returns `new_mean`,
        `new_sigma` [T][G][N][2] (sigma at least sigma_min), `best`, `best_score` [G] and `order`
        [G][elites] (elites) or `weights` [C] (softmax).  device=True: device tensors/pointers, only
        the outputs present in `out` are written, T and C from actions.shape (or `length` / `groups`)."""
        N, K = self.N, int(samples)
        if mode not in ("elites", "softmax"):
            raise ValueError(f"mode must be 'elites' or 'softmax', got {mode!r}")
        el = mode == "elites"
        M = int(elites) if elites is not None else max(1, K // 4)
        if device:
            shp = getattr(actions, "shape", None)
            if length is None and shp is not None:
                length = shp[0]
            if groups is None and shp is not None:
                groups = shp[1] // K
            if length is None or groups is None:
                raise ValueError("update_plans needs actions [T][C][N][2] (or length=T, groups=G)")
            T, G = int(length), int(groups)
            out = out if out is not None else {}
        else:
            actions = np.ascontiguousarray(actions, np.float32)
            if actions.ndim != 4 or actions.shape[2:] != (N, 2) or actions.shape[1] % K:
                raise ValueError(f"actions must be [T][G * {K}][{N}][2], got {actions.shape}")
            T, G = int(actions.shape[0]), int(actions.shape[1]) // K
            C = G * K
            if scores is not None:
                scores = np.ascontiguousarray(scores, np.float32)
                if scores.shape != (C,):
                    raise ValueError(f"scores must be [{C}], got {scores.shape}")
            if returns is not None:
                returns = np.ascontiguousarray(returns, np.float32)
                if returns.shape != (C, N):
                    raise ValueError(f"returns must be [{C}][{N}], got {returns.shape}")
            shapes = {"new_mean": ((T, G, N, 2), np.float32), "new_sigma": ((T, G, N, 2), np.float32),
                      "best": ((G,), np.int32), "best_score": ((G,), np.float32)}
            shapes.update({"order": ((G, M), np.int32)} if el else {"weights": ((C,), np.float32)})
            out = out if out is not None else {}
            if not out:
                for k, (shape, dtype) in shapes.items():
                    out[k] = np.zeros(shape, dtype)
            for k, (shape, dtype) in shapes.items():
                if out.get(k) is not None and (out[k].shape != shape or out[k].dtype != dtype):
                    raise ValueError(f"{k} must be {np.dtype(dtype).name} {list(shape)}, got {out[k].shape}")
        ua = MevUpdateArgs()
        ua.actions, ua.scores, ua.returns = _ptr(actions), _ptr(scores), _ptr(returns)
        ua.groups, ua.samples, ua.length = G, K, T
        ua.mode, ua.elites = (MEV_UPDATE_ELITES, M) if el else (MEV_UPDATE_SOFTMAX, 0)
        t = float(temperature)
        ua.inv_temperature = (0.0 if t == float("inf") else 1.0 / t) if t != 0.0 else float("inf")
        ua.sigma_min = float(sigma_min)
        for k in ("new_mean", "new_sigma", "best", "best_score", "order", "weights"):
            setattr(ua, k, _ptr(out.get(k)))
        ua.flags = (MEV_DEVICE_PTRS if device else 0) | int(flags)
        _check(self._lib.mev_update_plans(self._h, ctypes.byref(ua)))
        return out

    # -- multi-GPU gather (mev_comm_*) -------------------------------------
    def comm_init(self, unique_id: bytes, world: int, rank: int, root: int = 0, slots: int = 0):
        """Join the RCCL communicator (collective over all ranks); slots = envs of the largest shard."""
        if len(unique_id) != MEV_COMM_ID_BYTES:
            raise ValueError("unique_id must be MEV_COMM_ID_BYTES bytes")
        _check(self._lib.mev_comm_init(self._h, bytes(unique_id), int(world), int(rank), int(root), int(slots)))
        self.comm = dict(world=int(world), rank=int(rank), root=int(root), slots=int(slots) or self.E)

    def set_gather_format(self, fmt: int):
        """MEV_GATHER_F32 (plain obs rows), MEV_GATHER_LIDAR_U8 (31-float heads + one LiDAR code per
        beam) or MEV_GATHER_STATE (post-step state + LiDAR codes, the heads rebuilt on the root);
        all lossless; before comm_init."""
        _check(self._lib.mev_set_gather_format(self._h, int(fmt)))
        self.gather_format = int(fmt)

    def lidar_decode_table(self) -> np.ndarray:
        """The compact gather format's 256-entry code -> LiDAR float table (mev_lidar_decode_table)."""
        t = np.zeros(256, np.float32)
        _check(self._lib.mev_lidar_decode_table(self._h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return t

    def lidar_slots(self) -> int:
        return min(self.R, self.D - 31)

    def comm_destroy(self):
        _check(self._lib.mev_comm_destroy(self._h))
        self.comm = None

    def gather_result(self):
        """Root: (device pointer, bytes per rank, world) of the last gathered step's [world][bytes] buffer;
        the handle's stream is made to wait for that gather."""
        p, n, w = _vp(), ctypes.c_uint64(), ctypes.c_int32()
        _check(self._lib.mev_gather_result(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(w)))
        return p.value, n.value, w.value

    def gather_wait(self, timeout_ms: int = 0):
        """Host wait for every gather issued so far (timeout: the communicator is aborted, MevError)."""
        _check(self._lib.mev_gather_wait(self._h, int(timeout_ms)))

    def unpack_gathered(self, stacked_ptr: int, world: int, obs_ptr: int):
        """Root: the float observation rows [world][slots][N][D] (device, obs_ptr) of a gathered
        [world][bytes] device buffer in this handle's format (mev_unpack_gathered, on its stream)."""
        _check(self._lib.mev_unpack_gathered(self._h, _vp(int(stacked_ptr)), int(world), _vp(int(obs_ptr))))

    # -- zero-copy export (DLPack) ----------------------------------------
    def output_dlpack(self, which: str):
        """PyCapsule ("dltensor") viewing the handle's internal output buffer `which` (DLPACK_OUTPUTS);
        valid while the handle lives; torch.from_dlpack() consumes it.  A capsule dropped unconsumed
        frees its descriptor through the capsule destructor (DLPack's producer contract)."""
        m = _vp()
        _check(self._lib.mev_output_dlpack(self._h, DLPACK_OUTPUTS.index(which), ctypes.byref(m)))
        new = ctypes.pythonapi.PyCapsule_New
        new.restype = ctypes.py_object
        new.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
        return new(m.value, _DLTENSOR, ctypes.cast(_capsule_destructor, ctypes.c_void_p))

    def output_tensors(self, names=("obs", "reward", "done", "status", "terminated", "truncated",
                                    "agents_alive", "step")):
        """The internal output buffers as torch tensors (zero copy, through DLPack)."""
        import torch.utils.dlpack as tdl
        return {k: tdl.from_dlpack(self.output_dlpack(k)) for k in names}

    def get_outputs(self, out: Optional[dict] = None, device: bool = False):
        """Outputs of the last step/reset/restore; device=True: `out` holds device buffers (D2D copies)."""
        out = out or self.alloc_outputs()
        _check(self._lib.mev_get_outputs(self._h, *[_ptr(out.get(k)) for k in (
            "obs", "reward", "done", "status", "terminated", "truncated", "agents_alive", "step")],
            MEV_DEVICE_PTRS if device else 0))
        return out

    def observations(self) -> np.ndarray:
        obs = np.zeros((self.E, self.N, self.D), np.float32)
        _check(self._lib.mev_get_outputs(self._h, _ptr(obs), None, None, None, None, None, None, None, 0))
        return obs

    # -- state ------------------------------------------------------------
    def _shape(self, per):
        return {"ego": (self.E, self.N), "npc": (self.E, self.K), "env": (self.E,)}[per]

    def get_state(self) -> Dict[str, np.ndarray]:
        st = MevState()
        arrays = {}
        for name, dt, per in STATE_FIELDS:
            a = np.zeros(self._shape(per), dt)
            arrays[name] = a
            setattr(st, name, _ptr(a) if a.size else None)
        _check(self._lib.mev_get_state(self._h, ctypes.byref(st)))
        return arrays

    def set_state(self, state: Dict[str, np.ndarray]):
        st = MevState()
        keep = []
        for name, dt, per in STATE_FIELDS:
            if name in state and state[name] is not None:
                a = np.ascontiguousarray(np.broadcast_to(np.asarray(state[name], dt), self._shape(per)))
                if a.size == 0:
                    continue
                keep.append(a)
                setattr(st, name, _ptr(a))
        _check(self._lib.mev_set_state(self._h, ctypes.byref(st)))

    def configure(self, use_team: bool, respawn: bool, max_steps: int):
        _check(self._lib.mev_configure(self._h, int(use_team), int(respawn), int(max_steps)))
        self.config.update(use_team_reward=int(use_team), respawn_enabled=int(respawn), max_steps=int(max_steps))

    def configure_traffic(self, enabled: bool, density: float):
        _check(self._lib.mev_configure_traffic(self._h, int(enabled), float(density)))
        self.config.update(traffic_flow=int(enabled), traffic_density=max(0.0, float(density)))

    def set_reward(self, reward):
        rc = np.ascontiguousarray(reward, np.float32)
        assert rc.size == 8
        _check(self._lib.mev_set_reward(self._h, rc.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        self.config["reward"] = [float(x) for x in rc]

    def kernel_timing(self, every: int = 1):
        """Record per-kernel HIP events on every `every`-th step (0/False: off)."""
        _check(self._lib.mev_kernel_timing(self._h, int(every)))

    def kernel_times(self):
        """(k_cars ms summed, k_lidar ms summed, timed steps) since the previous call."""
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _check(self._lib.mev_kernel_times(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    def set_step_kernel(self, kernel: int = 0):
        """0: automatic, 1: k_cars + k_lidar, 2: the fused k_step (scheduling only; results identical)."""
        _check(self._lib.mev_set_step_kernel(self._h, int(kernel)))

    def step_kernel(self) -> int:
        """The kernel path the next step uses: 1 (k_cars + k_lidar) or 2 (fused k_step)."""
        v = ctypes.c_int32()
        _check(self._lib.mev_get_step_kernel(self._h, ctypes.byref(v)))
        return v.value

    def set_step_pack(self, envs_per_wave: int = 0):
        """Envs per fused k_step wave: 0 automatic, 1, 2, 4 or 8 (scheduling only; results identical)."""
        _check(self._lib.mev_set_step_pack(self._h, int(envs_per_wave)))

    def step_pack(self) -> int:
        """Envs per wave the next step uses (1 on the two-kernel path)."""
        v = ctypes.c_int32()
        _check(self._lib.mev_get_step_pack(self._h, ctypes.byref(v)))
        return v.value

    def set_step_split(self, mode: int = 0):
        """Two waves per fused workgroup: 0 automatic, 1 off, 2 on, 3 early split (scheduling only;
        results identical)."""
        _check(self._lib.mev_set_step_split(self._h, int(mode)))

    def set_env_deal(self, on: bool = True):
        """The fused traffic kernel's NPC-aware env deal on / off (scheduling only; results identical)."""
        _check(self._lib.mev_set_env_deal(self._h, 1 if on else 0))

    def step_split(self) -> int:
        """Two waves per fused workgroup in the next step: 0 no, 1 split, 2 early split."""
        v = ctypes.c_int32()
        _check(self._lib.mev_get_step_split(self._h, ctypes.byref(v)))
        return int(v.value)

    def step_row(self) -> dict:
        """The compiled kernels this handle runs (mev_get_step_row): `step`, the k_step row (kStepKeys,
        csrc/mev_plan.h) of the next launched step into the handle's own buffers, -1 on the two-kernel
        path; `serve`, the k_serve row (kServeKeys) of the persistent step server, -1 where it does
        not apply; `tab`, 1 when the kernels read the probe distances from a table."""
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.mev_get_step_row(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"step": int(a.value), "serve": int(b.value), "tab": int(c.value)}

    def set_serve(self, mode: int = 1):
        """Host-mode steps through the persistent step server: 0 off, 1 automatic (results identical)."""
        _check(self._lib.mev_set_serve(self._h, int(mode)))

    def serve_stats(self) -> dict:
        """Steps the persistent server answered, its launches, and whether one is running."""
        st, la, ru = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int32()
        _check(self._lib.mev_serve_stats(self._h, ctypes.byref(st), ctypes.byref(la), ctypes.byref(ru)))
        return {"steps": int(st.value), "launches": int(la.value), "running": bool(ru.value)}

    def set_reset_routes(self, routes):
        """Draw every agent's route from `routes` at each reset (empty: fixed routes)."""
        r = np.ascontiguousarray(np.asarray(routes, np.int32).reshape(-1))
        _check(self._lib.mev_set_reset_routes(self._h, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if r.size
                                              else None, int(r.size)))

    def snapshot_size(self) -> int:
        n = ctypes.c_uint64()
        _check(self._lib.mev_snapshot_size(self._h, ctypes.byref(n)))
        return n.value

    def snapshot(self, dst=None, device: bool = False):
        """Whole-state snapshot into `dst` (host uint8 array, or a device buffer/tensor with device=True)."""
        if dst is None:
            if device:
                raise ValueError("device snapshots need a caller-provided device buffer")
            dst = np.zeros(self.snapshot_size(), np.uint8)
        _check(self._lib.mev_snapshot(self._h, _ptr(dst), MEV_DEVICE_PTRS if device else 0))
        return dst

    def restore(self, src, env_mask=None, device: bool = False, env_map=None):
        """Roll every env (or those with env_mask != 0) back to snapshot `src`; or, with env_map
        ([E] int32), give env e the state, car sizes and last outputs of the snapshot's env
        env_map[e] (-1: leave env e alone) -- mev_restore_map, a planner's branching."""
        if env_map is not None:
            if env_mask is not None:
                raise ValueError("pass env_mask or env_map, not both")
            if not device:
                env_map = np.ascontiguousarray(env_map, np.int32)
                if env_map.shape != (self.E,):
                    raise ValueError(f"env_map must have {self.E} entries, got {env_map.shape}")
            _check(self._lib.mev_restore_map(self._h, _ptr(src), _ptr(env_map), MEV_DEVICE_PTRS if device else 0))
            return
        mask = None if env_mask is None else (env_mask if device else np.ascontiguousarray(env_mask, np.uint8))
        _check(self._lib.mev_restore(self._h, _ptr(src), _ptr(mask), MEV_DEVICE_PTRS if device else 0))

    def npc_stats(self):
        """(dropped spawns, NPC turns run sequentially after a parallel-round disagreement), cumulative."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _check(self._lib.mev_npc_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def decode_errors(self) -> int:
        """Route ids of state-format gather messages this handle's route table lacks (cumulative)."""
        v = ctypes.c_int64()
        _check(self._lib.mev_decode_errors(self._h, ctypes.byref(v)))
        return v.value

    # -- per-car sizes and beam angles -------------------------------------
    def set_car_dims(self, ego=None, npc=None):
        """Car::length / Car::width of every ego ([E][N][2]) and NPC slot ([E][K][2]) in px (mev_set_car_dims);
        None leaves that array as it is."""
        f32p = ctypes.POINTER(ctypes.c_float)
        e = None if ego is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ego, np.float32),
                                                                          (self.E, self.N, 2)))
        n = None if npc is None else np.ascontiguousarray(np.broadcast_to(np.asarray(npc, np.float32),
                                                                          (self.E, self.K, 2)))
        _check(self._lib.mev_set_car_dims(self._h, None if e is None else e.ctypes.data_as(f32p),
                                          None if n is None or n.size == 0 else n.ctypes.data_as(f32p)))

    def car_dims(self):
        """(ego [E][N][2], NPC [E][K][2]) (length, width) of every car."""
        f32p = ctypes.POINTER(ctypes.c_float)
        e = np.zeros((self.E, self.N, 2), np.float32)
        n = np.zeros((self.E, self.K, 2), np.float32)
        _check(self._lib.mev_get_car_dims(self._h, e.ctypes.data_as(f32p), n.ctypes.data_as(f32p) if n.size else None))
        return e, n

    def car_dims_active(self) -> bool:
        """Whether some car differs from the reference's 54 x 24 px (the steps then run the runtime-layout kernels)."""
        v = ctypes.c_int32()
        _check(self._lib.mev_car_dims_active(self._h, ctypes.byref(v)))
        return bool(v.value)

    def set_beam_angles(self, rel):
        """LiDAR beam offsets [R] in radians (Lidar::rel_angles; evenly spaced)."""
        a = np.ascontiguousarray(np.asarray(rel, np.float32).reshape(-1))
        if a.size != self.R:
            raise ValueError(f"{self.R} beam angles expected, got {a.size}")
        _check(self._lib.mev_set_beam_angles(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))

    def beam_angles(self) -> np.ndarray:
        a = np.zeros(self.R, np.float32)
        _check(self._lib.mev_get_beam_angles(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return a

    def npc_overflow(self) -> int:
        v = ctypes.c_int64()
        _check(self._lib.mev_npc_overflow(self._h, ctypes.byref(v)))
        return v.value


class Pool:
    """A state pool of a Handle (mev_pool_create): `slots` env states on the device outside the live
    batch.  The handle's close() releases it too; close() after that is a no-op."""

    def __init__(self, handle: "Handle", slots: int):
        self._handle = handle
        self._lib = handle._lib
        p = _vp()
        _check(self._lib.mev_pool_create(handle._h, int(slots), ctypes.byref(p)))
        self._ptr = p.value
        n = ctypes.c_int32()
        _check(self._lib.mev_pool_slots(self._ptr, ctypes.byref(n)))
        self.slots = n.value

    @property
    def _p(self):
        if not self._ptr or not self._handle._h:
            raise MevError("the pool (or its handle) is closed")
        return self._ptr

    def close(self):
        if getattr(self, "_ptr", None) and self._handle._h:  # (a closed handle has released its pools)
            self._lib.mev_pool_destroy(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def capture(self, envs, slots, device: bool = False, count: Optional[int] = None):
        """Copy live env envs[i] into slot slots[i] without stepping (mev_pool_capture)."""
        if not device:
            envs = np.ascontiguousarray(envs, np.int32).reshape(-1)
            slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
            if envs.shape != slots.shape:
                raise ValueError(f"envs and slots must have one length, got {envs.size} and {slots.size}")
        n = int(count) if count is not None else int(getattr(envs, "shape", (0,))[0])
        _check(self._lib.mev_pool_capture(self._handle._h, self._p, _ptr(envs), _ptr(slots), n,
                                          MEV_DEVICE_PTRS if device else 0))

    def get_state(self, slots):
        """Host read-back of the given slots (mev_pool_get_state): (state dict as Handle.get_state with
        rows = the slots, (ego_dims [n][N][2], npc_dims [n][K][2]), valid [n])."""
        h = self._handle
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = int(slots.size)
        shape = {"ego": (n, h.N), "npc": (n, h.K), "env": (n,)}
        st, arrays = MevState(), {}
        for name, dt, per in STATE_FIELDS:
            a = np.zeros(shape[per], dt)
            arrays[name] = a
            setattr(st, name, _ptr(a) if a.size else None)
        ed, nd = np.zeros((n, h.N, 2), np.float32), np.zeros((n, h.K, 2), np.float32)
        valid = np.zeros(n, np.uint8)
        _check(self._lib.mev_pool_get_state(self._p, _ptr(slots), n, ctypes.byref(st), _ptr(ed),
                                            _ptr(nd) if nd.size else None, _ptr(valid)))
        return arrays, (ed, nd), valid


class Policy:
    """An MLP policy of a handle (mev_policy): 1 or 2 hidden layers of <= MEV_POLICY_MAX_WIDTH units and 2
    outputs, kept on the device in the library's own layout.  `update` takes new weights of the same
    shape; Handle.close releases a policy that was not closed."""

    def __init__(self, handle: "Handle", weights, biases, device: bool = False, hidden: str = "relu",
                 out: str = "linear"):
        self._handle = handle
        self._ptr = None
        p = _vp()
        flags = (MEV_DEVICE_PTRS if device else 0) | activation_flags(hidden, out)
        spec, _keep = self._spec(weights, biases, device)
        _check(handle._lib.mev_policy_create(handle._h, ctypes.byref(spec), flags, ctypes.byref(p)))
        self._ptr = p

    def _spec(self, weights, biases, device):
        weights, biases = list(weights), list(biases)
        if len(weights) not in (2, 3) or len(biases) != len(weights):
            raise ValueError("a policy has 2 or 3 layers: as many weight arrays as bias arrays")
        if not device:
            weights = [np.ascontiguousarray(w, np.float32) for w in weights]
            biases = [np.ascontiguousarray(b, np.float32) for b in biases]
        shapes = [tuple(int(x) for x in w.shape) for w in weights]
        if any(len(sh) != 2 for sh in shapes) or shapes[-1][0] != 2:
            raise ValueError(f"weights must be [out][in] arrays, the last with 2 outputs, got {shapes}")
        for l, (sh, b) in enumerate(zip(shapes, biases)):
            if tuple(int(x) for x in b.shape) != (sh[0],) or (l and sh[1] != shapes[l - 1][0]):
                raise ValueError(f"layer {l}: weights {sh} do not fit the bias {tuple(b.shape)} or the layer before")
        if getattr(self, "shapes", shapes) != shapes:
            raise ValueError(f"update needs the policy's own shape {self.shapes}, got {shapes}")
        self.shapes = shapes
        spec = MevPolicySpec()
        spec.in_dim = shapes[0][1]
        spec.hidden[0] = shapes[0][0]
        spec.hidden[1] = shapes[1][0] if len(shapes) == 3 else 0
        for l, (w, b) in enumerate(zip(weights, biases)):
            spec.w[l], spec.b[l] = _ptr(w), _ptr(b)
        return spec, (weights, biases)

    @property
    def _p(self):
        if self._ptr is None or not self._handle._h:
            raise MevError("the policy (or its handle) is closed")
        return self._ptr

    def update(self, weights, biases, device: bool = False):
        """New weights of the same shape (mev_policy_update); device=True: stream-ordered, no host copy."""
        spec, _keep = self._spec(weights, biases, device)
        _check(self._handle._lib.mev_policy_update(self._p, ctypes.byref(spec), MEV_DEVICE_PTRS if device else 0))

    def set_value_head(self, w, b, device: bool = False):
        """Attach a value head on the last hidden layer (mev_policy_set_value_head): w [H_last] (or [1][H_last],
        nn.Linear(H_last, 1).weight), b [1]; w None detaches it.  device=True: stream-ordered, no host copy.
        `update` leaves an attached head as it is."""
        if w is not None:
            H = self.shapes[-1][1]
            if not device:
                w = np.ascontiguousarray(w, np.float32).reshape(-1)
                b = np.ascontiguousarray(b, np.float32).reshape(-1)
            n = 1
            for x in w.shape:
                n *= int(x)
            nb = 1
            for x in b.shape:
                nb *= int(x)
            if n != H or nb != 1:
                raise ValueError(f"a value head has {H} weights and 1 bias, got {tuple(w.shape)} and {tuple(b.shape)}")
        _check(self._handle._lib.mev_policy_set_value_head(self._p, _ptr(w) if w is not None else None,
                                                           _ptr(b) if w is not None else None,
                                                           MEV_DEVICE_PTRS if device else 0))

    @property
    def has_value_head(self) -> bool:
        has = ctypes.c_int32()
        _check(self._handle._lib.mev_policy_has_value_head(self._p, ctypes.byref(has)))
        return bool(has.value)

    @property
    def activations(self):
        """(hidden, out) as given at creation: ("relu" | "tanh", "linear" | "tanh") (mev_policy_get_activations)."""
        f = ctypes.c_uint32()
        _check(self._handle._lib.mev_policy_get_activations(self._p, ctypes.byref(f)))
        return ("tanh" if f.value & MEV_POLICY_HIDDEN_TANH else "relu",
                "tanh" if f.value & MEV_POLICY_OUT_TANH else "linear")

    def close(self):
        if self._ptr is not None and self._handle._h:
            self._handle._lib.mev_policy_destroy(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def activation_flags(hidden: str = "relu", out: str = "linear") -> int:
    """mev_policy_create's activation bits for hidden in ("relu", "tanh") and out in ("linear", "tanh")."""
    if hidden not in ("relu", "tanh"):
        raise ValueError(f'hidden must be "relu" or "tanh", got {hidden!r}')
    if out not in ("linear", "tanh"):
        raise ValueError(f'out must be "linear" or "tanh", got {out!r}')
    return (MEV_POLICY_HIDDEN_TANH if hidden == "tanh" else 0) | (MEV_POLICY_OUT_TANH if out == "tanh" else 0)


def tanh_c(x):
    """tanh_c of every element (mev_tanh): the rollout policies' tanh, the library's stated f32 arithmetic run on
    the host -- the same bits as inside the kernels.  Returns a float32 array of x's shape."""
    a = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(a)
    f32p = ctypes.POINTER(ctypes.c_float)
    _check(load_library().mev_tanh(a.ctypes.data_as(f32p), y.ctypes.data_as(f32p), a.size))
    return y


def car_update(kin, throttle: float, steer: float, dt: float):
    """Host Car::update with the reference's exact arithmetic; kin = [x, y, v, heading, acc, steering]."""
    k = np.ascontiguousarray(kin, np.float32).copy()
    _check(load_library().mev_car_update(k.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(throttle),
                                         float(steer), float(dt)))
    return k


def car_check_collision(box_a, box_b) -> bool:
    """Host Car::check_collision; box = [x, y, heading, length, width]."""
    a = np.ascontiguousarray(box_a, np.float32)
    b = np.ascontiguousarray(box_b, np.float32)
    r = ctypes.c_int32()
    _check(load_library().mev_car_check_collision(a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(r)))
    return bool(r.value)


def packed_layout(slots: int, agents: int, obs_dim: int, fmt: int = MEV_GATHER_F32, lidar_slots: int = 0):
    """(offsets by field, total bytes) of one rank's packed outputs (mev_packed_layout2; host-only, no GPU).
    fmt MEV_GATHER_LIDAR_U8: "obs" holds [slots][N][31] heads and "lidar" [slots][N][lidar_slots] codes;
    MEV_GATHER_STATE: "obs" is empty, "state" holds the post-step state arrays (22 B per agent)."""
    off = (ctypes.c_uint64 * len(PACKED_FIELDS))()
    n = ctypes.c_uint64()
    _check(load_library().mev_packed_layout2(int(slots), int(agents), int(obs_dim), int(lidar_slots), int(fmt), off,
                                             ctypes.byref(n)))
    return dict(zip(PACKED_FIELDS, (int(x) for x in off))), int(n.value)


def comm_unique_id() -> bytes:
    """ncclGetUniqueId (call on ONE rank, share the bytes with all)."""
    _torch_runtime_first()
    buf = ctypes.create_string_buffer(MEV_COMM_ID_BYTES)
    _check(load_library().mev_comm_unique_id(buf))
    return buf.raw


def device_count() -> int:
    _torch_runtime_first()
    n = ctypes.c_int32()
    load_library().mev_device_count(ctypes.byref(n))
    return n.value
