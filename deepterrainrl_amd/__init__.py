"""deepterrainrl_amd -- MI355X-native batched rollout engine for the DeepTerrainRL environments.

Python host-side mirror of the reference's scenario interface for the rollout path, bound over the C ABI of
``include/dtrl.h`` with ctypes (plain pointers and sizes, no torch types cross the boundary).

    cScenarioExp / cScenarioPoliEval (one env)        ->  BatchScenario (N envs, one HIP device)
      ParseArgs + Init                                  ->  BatchScenario(arg_file=..., num_envs=...)
      Update(dt)                                        ->  .Update(dt)
      Reset()                                           ->  .Reset(env_ids=None)
      IsTupleBufferFull/GetTuples/ResetTupleBuffer      ->  .DrainTuples()
      EnableExplore/SetExpRate/SetExpTemp/...           ->  .SetExplore(enable, rate, temp, base_rate)
      SetTerrainParamsLerp                              ->  .SetTerrainParamsLerp(lerp)
      GetCharacter()->BuildPose/BuildVel/SetPose/SetVel ->  .BuildPose() / .BuildVel() / .SetPoseVel()
      GetNNController()->RecordPoliState / LoadNet...   ->  .RecordPoliState() / .SetPolicy(weights, scales)
      GetAvgDist/GetNumEpisodes/GetNumCycles            ->  .EvalStats()

The product path is the HIP library ``lib/libdtrl.so``; importing works anywhere, but constructing a BatchScenario
raises ``DtrlError`` when the library or a HIP device is missing -- there is no CPU fallback.
"""
import os as _os
import sys as _sys
import warnings as _warnings


def configure_hw_queues(n=8):
    """Opt-in: ask HIP for `n` hardware queues (GPU_MAX_HW_QUEUES) unless the user has set the variable. The engine drives its env groups on separate
    HIP streams that must not share a hardware queue: HIP multiplexes all streams of a process onto 4 queues by default, and with RCCL's and a
    framework's streams in the same process the two groups' frame kernels ended up serialised (11.2 M instead of 19.1 M env-steps/s).
    The variable is read when the HIP runtime starts, so call this before the first device call of the PROCESS (bench.py and the training tools do);
    importing the package no longer touches the process environment. Returns the value in effect for a runtime that starts after this call."""
    return int(_os.environ.setdefault("GPU_MAX_HW_QUEUES", str(int(n))))


def _warn_hw_queues():
    """Called when a batch is created: with a framework in the process and the default queue count the env-group streams may share a queue."""
    v = _os.environ.get("GPU_MAX_HW_QUEUES")
    if "torch" in _sys.modules and (v is None or int(v) < 8):
        _warnings.warn("GPU_MAX_HW_QUEUES is %s: with torch / RCCL streams in this process the engine's env-group streams may share a HIP hardware queue and "
                       "serialise; call deepterrainrl_amd.configure_hw_queues() (or export GPU_MAX_HW_QUEUES=8) before the HIP runtime starts" % (v or "unset (4)"),
                       RuntimeWarning, stacklevel=3)


import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdtrl.so")
LIB_PATH_F32 = os.path.join(_HERE, "lib", "libdtrl_f32.so")   # the opt-in fp32 build of the same source (-physics_precision= f32): distribution-level parity only

DTRL_OK = 0
FLAG_FALLEN, FLAG_STUMBLED, FLAG_NEW_CYCLE, FLAG_STATE_SHIFT = 1, 2, 4, 8
TUPLE_FAIL, TUPLE_EXP_CRITIC, TUPLE_EXP_ACTOR = 1, 2, 4

# every symbol include/dtrl.h declares (tests check the built library exports all of them)
ABI_SYMBOLS = [
    "dtrl_create", "dtrl_destroy", "dtrl_reset", "dtrl_step", "dtrl_step_begin", "dtrl_step_end", "dtrl_step_updates", "dtrl_run_frames", "dtrl_set_policy",
    "dtrl_policy_num_params", "dtrl_build_output_offset_scale", "dtrl_load_scale_file", "dtrl_write_scale_file", "dtrl_set_explore", "dtrl_set_terrain_lerp", "dtrl_drain_tuples",
    "dtrl_get_pose_vel", "dtrl_set_pose_vel", "dtrl_get_contact_cache", "dtrl_set_contact_cache", "dtrl_get_link_states", "dtrl_add_perturb", "dtrl_apply_rand_force", "dtrl_get_cycle_info", "dtrl_get_action_table", "dtrl_get_poli_state", "dtrl_get_flags", "dtrl_get_torques", "dtrl_get_contacts",
    "dtrl_get_ctrl", "dtrl_sample_ground", "dtrl_eval_stats", "dtrl_dims", "dtrl_kernel_time_ms", "dtrl_last_error", "dtrl_version",
    "dtrl_terrain_build", "dtrl_terrain_load_file", "dtrl_args_parse_string",
    "dtrl_drain_tuples_device", "dtrl_tuple_stats", "dtrl_set_policy_device", "dtrl_get_dist_log", "dtrl_reset_avg_dist", "dtrl_write_dist_log", "dtrl_get_ground_window", "dtrl_drain_tuples_packed", "dtrl_get_policy_output", "dtrl_set_tuple_pipelining", "dtrl_step_end_begin", "dtrl_command_action", "dtrl_side_stream", "dtrl_step_poll", "dtrl_set_policy_device_on", "dtrl_set_policy_device_async",
    "dtrl_snapshot_save", "dtrl_snapshot_restore", "dtrl_clone_envs", "dtrl_snapshot_export", "dtrl_snapshot_import", "dtrl_snapshot_info", "dtrl_snapshot_free",
    "dtrl_slots_create", "dtrl_slot_set_policy", "dtrl_slot_set_policy_device", "dtrl_slot_alias", "dtrl_slot_set_explore", "dtrl_assign_slots", "dtrl_get_slots", "dtrl_slot_stats",
    "dtrl_variants_create", "dtrl_variant_load_file", "dtrl_variant_load_json", "dtrl_assign_variants", "dtrl_get_variants", "dtrl_variant_stats", "dtrl_variant_redraw", "dtrl_variant_redraw_info",
    "dtrl_variant_rescale", "dtrl_variant_rescale_info", "dtrl_variant_scalars",
    "dtrl_push_schedule", "dtrl_push_scale", "dtrl_push_info",
    "dtrl_episode_limit", "dtrl_episode_limit_envs", "dtrl_episode_info",
    "dtrl_trace", "dtrl_trace_info", "dtrl_trace_read", "dtrl_trace_read_device",
    "dtrl_episode_log", "dtrl_episode_log_info", "dtrl_episode_log_drain", "dtrl_variant_rescale_factors",
    "dtrl_terrains_create", "dtrl_terrain_set_file", "dtrl_terrain_set_params", "dtrl_terrain_info", "dtrl_assign_terrains", "dtrl_get_terrains", "dtrl_terrain_stats", "dtrl_terrain_ladder", "dtrl_ladder_info",
    "dtrl_pending_actions", "dtrl_pending_actions_device", "dtrl_supply_actions", "dtrl_supply_actions_device", "dtrl_ext_stats", "dtrl_ext_env_info", "dtrl_action_dims", "dtrl_ext_launch_ms",
]


class DtrlError(RuntimeError):
    pass


class RescaleDesc(C.Structure):
    """include/dtrl.h dtrl_rescale_desc: the four ranges {lo, hi} of the variant rescale and its per_link mask"""
    _fields_ = [("mass", C.c_double * 2), ("kp", C.c_double * 2), ("kd", C.c_double * 2), ("torque_lim", C.c_double * 2), ("per_link", C.c_uint32), ("reserved", C.c_uint32)]


RESCALE_QUANTITIES = ("mass", "kp", "kd", "torque_lim")   # the order of the per_link bits and of the factor rows
RESCALE_SCALARS = ("mass", "inertia", "sub_mass", "kp", "kd", "torque_lim")   # the rows of dtrl_variant_scalars


def _bind(path):
    if not os.path.exists(path):
        raise DtrlError("HIP extension missing: %s (run __graft_entry__.build() / make -C deepterrainrl_amd/csrc)" % path)
    L = C.CDLL(path)
    vp, i32p, u32p, u64p, dp, fp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.dtrl_create.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.dtrl_destroy.argtypes = [vp]
    L.dtrl_reset.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_step.argtypes = [vp, C.c_double]
    L.dtrl_step_begin.argtypes = [vp, C.c_double]
    L.dtrl_step_end.argtypes = [vp]
    L.dtrl_step_updates.argtypes = [vp, C.c_int]
    L.dtrl_run_frames.argtypes = [vp, C.c_int, C.c_double]
    L.dtrl_set_policy.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp]
    L.dtrl_policy_num_params.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.dtrl_build_output_offset_scale.argtypes = [vp, vp, vp]
    L.dtrl_load_scale_file.argtypes = [vp, C.c_char_p]
    L.dtrl_write_scale_file.argtypes = [vp, C.c_char_p]
    L.dtrl_set_explore.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    L.dtrl_set_terrain_lerp.argtypes = [vp, C.c_double]
    L.dtrl_drain_tuples.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    for name in ("dtrl_get_pose_vel", "dtrl_get_torques"):
        getattr(L, name).argtypes = [vp, vp, C.c_int, vp, vp]
    L.dtrl_set_pose_vel.argtypes = [vp, vp, C.c_int, vp, vp]
    L.dtrl_get_contact_cache.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.dtrl_set_contact_cache.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.dtrl_command_action.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_side_stream.restype = C.c_void_p; L.dtrl_side_stream.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.dtrl_get_link_states.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.dtrl_add_perturb.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.dtrl_apply_rand_force.argtypes = [vp, vp, C.c_int, C.c_uint64]
    L.dtrl_get_cycle_info.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.dtrl_get_action_table.argtypes = [vp, C.POINTER(C.c_int), vp]
    L.dtrl_get_poli_state.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_get_policy_output.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_set_tuple_pipelining.argtypes = [vp, C.c_int]
    L.dtrl_step_end_begin.argtypes = [vp, C.c_double]
    L.dtrl_step_poll.argtypes = [vp, C.c_double, C.POINTER(C.c_int)]
    L.dtrl_get_flags.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_get_contacts.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_get_ctrl.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.dtrl_sample_ground.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.dtrl_drain_tuples_packed.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_get_ground_window.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int64)]
    L.dtrl_eval_stats.argtypes = [vp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dtrl_dims.argtypes = [vp] + [C.POINTER(C.c_int)] * 8
    L.dtrl_kernel_time_ms.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    L.dtrl_terrain_build.argtypes = [C.c_char_p, vp, C.c_uint64, C.c_double, vp, C.c_int, C.POINTER(C.c_int), dp]
    L.dtrl_terrain_load_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_args_parse_string.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dtrl_drain_tuples_device.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_tuple_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.dtrl_set_policy_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp]
    L.dtrl_set_policy_device_on.argtypes = [vp, vp, C.c_size_t, vp]
    L.dtrl_set_policy_device_async.argtypes = [vp, vp, C.c_size_t, vp]
    L.dtrl_get_dist_log.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_reset_avg_dist.argtypes = [vp]
    L.dtrl_write_dist_log.argtypes = [vp, C.c_char_p]
    L.dtrl_snapshot_save.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.dtrl_snapshot_restore.argtypes = [vp, vp, vp, C.c_int]
    L.dtrl_clone_envs.argtypes = [vp, vp, vp, C.c_int]
    L.dtrl_snapshot_export.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dtrl_snapshot_import.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.dtrl_snapshot_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.dtrl_snapshot_free.argtypes = [vp]
    L.dtrl_pending_actions.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_pending_actions_device.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.dtrl_supply_actions.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.dtrl_supply_actions_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    L.dtrl_ext_stats.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
    L.dtrl_ext_env_info.argtypes = [vp, vp, C.c_int, vp, vp]
    L.dtrl_action_dims.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    L.dtrl_ext_launch_ms.restype = C.c_double; L.dtrl_ext_launch_ms.argtypes = [vp, C.c_int]
    L.dtrl_slots_create.argtypes = [vp, C.c_int]
    L.dtrl_slot_set_policy.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.dtrl_slot_set_policy_device.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    L.dtrl_slot_alias.argtypes = [vp, C.c_int, C.c_int]
    L.dtrl_slot_set_explore.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    L.dtrl_assign_slots.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_get_slots.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_slot_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dtrl_variants_create.argtypes = [vp, C.c_int]
    L.dtrl_variant_load_file.argtypes = [vp, C.c_int, C.c_char_p]
    L.dtrl_variant_load_json.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    L.dtrl_assign_variants.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_get_variants.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_variant_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dtrl_variant_redraw.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, vp]
    L.dtrl_variant_redraw_info.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.dtrl_variant_rescale.argtypes = [vp, C.c_int, vp, C.c_int, C.c_uint64, C.POINTER(RescaleDesc)]
    L.dtrl_variant_rescale_info.argtypes = [vp, vp, C.c_int, i32p, u64p, C.POINTER(RescaleDesc), vp, vp, vp]
    L.dtrl_variant_scalars.argtypes = [vp, C.c_int, vp, dp]
    L.dtrl_push_schedule.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double]
    L.dtrl_push_scale.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_push_info.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.dtrl_episode_limit.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint64]
    L.dtrl_episode_limit_envs.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_episode_info.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.dtrl_trace.argtypes = [vp, vp, C.c_int, C.c_int]
    L.dtrl_trace_info.argtypes = [vp, i32p, i32p, i32p, vp, vp]
    L.dtrl_trace_read.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.dtrl_trace_read_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.dtrl_episode_log.argtypes = [vp, C.c_int32]
    L.dtrl_episode_log_info.argtypes = [vp, i32p, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dtrl_episode_log_drain.argtypes = [vp, vp, C.c_int32, i32p, C.POINTER(C.c_int64)]
    L.dtrl_variant_rescale_factors.argtypes = [vp, vp, vp, C.c_int32, vp]
    L.dtrl_terrains_create.argtypes = [vp, C.c_int]
    L.dtrl_terrain_set_file.argtypes = [vp, C.c_int, C.c_char_p, C.c_double]
    L.dtrl_terrain_set_params.argtypes = [vp, C.c_int, C.c_char_p, vp]
    L.dtrl_terrain_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, vp, C.POINTER(C.c_int)]
    L.dtrl_assign_terrains.argtypes = [vp, vp, C.c_int, vp, C.c_int]
    L.dtrl_get_terrains.argtypes = [vp, vp, C.c_int, vp]
    L.dtrl_terrain_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dtrl_terrain_ladder.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    L.dtrl_ladder_info.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.dtrl_last_error.restype = C.c_char_p
    L.dtrl_last_error.argtypes = [vp]
    L.dtrl_version.restype = C.c_char_p
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# the layout of dtrl_episode_row (include/dtrl.h): what dtrl_episode_log_drain fills
EPISODE_ROW_DTYPE = np.dtype([("env", np.int32), ("cause", np.int32), ("frames", np.int32), ("cycles", np.int32), ("boundary", np.int64), ("episode", np.int64),
                              ("dist", np.float64), ("need_reset", np.int32), ("zero", np.int32), ("slot", np.int32), ("variant", np.int32), ("terrain", np.int32), ("rescale_draw", np.int32)])
assert EPISODE_ROW_DTYPE.itemsize == 64


# ---- env snapshots: the layout of dtrl_types.h EnvState and of dtrl_engine.h SnapHeader, for reading or editing an exported blob ----
_MAX_D, _MAX_L, _MAX_P, _MAX_ROWS = 24, 24, 40, 24


def env_state_dtype(real):
    """numpy structured dtype of `struct EnvState` (csrc/dtrl_types.h) for real = np.float64 (libdtrl.so) or np.float32 (libdtrl_f32.so), C alignment rules applied."""
    r = np.dtype(real)
    i32, u32, i64, u64 = np.int32, np.uint32, np.int64, np.uint64
    return np.dtype([
        ("q", r, _MAX_D), ("qd", r, _MAX_D), ("tau", r, _MAX_D), ("tau_ctrl", r, _MAX_D), ("pd_target", r, _MAX_L), ("params", r, _MAX_P),
        ("phase", r), ("curr_cycle_time", r), ("prev_cycle_time", r), ("prev_stumble", r), ("curr_stumble", r),
        ("prev_com", r, 2), ("prev_dist", r, 2), ("fall_dist_counter", r), ("fall_contact_counter", r), ("sum_fall_contact", r), ("prev_check", r, 2),
        ("sample_origin", r, 2), ("time", r), ("pos_start_x", r), ("avg_dist", r),
        ("rng_ctr", u64), ("num_cycles", i64), ("num_resets", i64), ("num_episodes", i64),
        ("action_id", i32), ("state", i32), ("first_cycle", i32), ("is_off_policy", i32),
        ("exp_actor", i32), ("exp_critic", i32), ("cmd_action", i32), ("fail_fall_dist", i32),
        ("stance", i32), ("pd_active_bits", u32), ("contact_bits", u32), ("cycle_count", i32), ("tuple_flags", i32),
        ("need_reset", i32), ("do_reset", i32), ("do_init", i32), ("pert_link", i32), ("pert_on", i32), ("ext_steps_left", i32),
        ("pert_f", r, 2), ("pert_lp", r, 2), ("pert_torque", r), ("pert_time", r), ("pert_dur", r),
        ("ws_lam", r, _MAX_ROWS), ("ws_id", np.uint16, _MAX_ROWS), ("ws_R", i32), ("ext_park", i32),
    ], align=True)


SNAP_MAGIC = 0x31504E534C525444   # "DTRLSNP1"
SNAP_HEADER_DTYPE = np.dtype([
    ("magic", np.uint64), ("version", np.uint32), ("header_bytes", np.uint32),
    ("sizeof_real", np.uint32), ("sizeof_env_state", np.uint32), ("sizeof_ground_rec", np.uint32), ("sizeof_ground_gen", np.uint32),
    ("sizeof_env_status", np.uint32), ("sizeof_ground_host", np.uint32),
    ("char_type", np.int32), ("ctrl_type", np.int32), ("L", np.int32), ("D", np.int32), ("S", np.int32), ("A", np.int32), ("nn_out", np.int32),
    ("terrain_mode", np.int32), ("env_bytes", np.uint32), ("host_bytes", np.uint32), ("n_envs", np.int32), ("policy_mode", np.int32)], align=True)


class Snapshot:
    """Everything that decides the future of a list of envs of one batch (include/dtrl.h: dtrl_snapshot_save), held by the library with its payload in device
    memory. Made by BatchScenario.SaveState / ImportState; goes back with RestoreState. Not held: policy, exploration settings, terrain lerp, tuple rings."""

    def __init__(self, batch, handle):
        self._b, self._h = batch, handle
        n = C.c_int32(); pe = C.c_size_t(); se = C.c_size_t(); he = C.c_size_t()
        batch._lib.dtrl_snapshot_info(handle, C.byref(n), C.byref(pe), C.byref(se), C.byref(he))
        self.num_envs, self.bytes_per_env, self.sizeof_env_state, self.host_bytes_per_env = n.value, pe.value, se.value, he.value

    def free(self):
        if getattr(self, "_h", None):
            self._b._lib.dtrl_snapshot_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def export(self):
        """The snapshot as one flat, self-describing host blob (bytes): header, saved slot ids, device payload, host payload."""
        n = C.c_size_t()
        self._b._chk(self._b._lib.dtrl_snapshot_export(self._h, None, 0, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        self._b._chk(self._b._lib.dtrl_snapshot_export(self._h, _p(buf), buf.size, C.byref(n)))
        return buf.tobytes()

    def env_ids(self):
        """The slots the envs were saved from, in saved order."""
        hdr, ids, _ = snapshot_blob_views(bytearray(self.export()))
        return ids.copy()

    def env_state(self, blob=None):
        """The EnvState section of an exported blob as a numpy structured array [num_envs] (env_state_dtype: FSM state, phase, timers, the soft-fall filter ...).
        Without an argument: a copy read from a fresh export. With a bytearray `blob` (bytearray(snap.export())): a writable VIEW into it -- edit fields, then
        BatchScenario.ImportState(blob) and RestoreState."""
        own = blob is None
        if own:
            blob = bytearray(self.export())
        _, _, st = snapshot_blob_views(blob)
        if st.dtype.itemsize != self.sizeof_env_state:
            raise DtrlError("env_state dtype is %d bytes, the library's EnvState %d" % (st.dtype.itemsize, self.sizeof_env_state))
        return st.copy() if own else st


def snapshot_blob_views(blob):
    """(header record, slot ids int32[n], EnvState records [n]) of an exported snapshot blob; views into `blob` when it is a bytearray (writable)."""
    raw = np.frombuffer(blob, np.uint8)
    if raw.size < SNAP_HEADER_DTYPE.itemsize:
        raise DtrlError("snapshot blob shorter than its header")
    hdr = raw[:SNAP_HEADER_DTYPE.itemsize].view(SNAP_HEADER_DTYPE)[0]
    if int(hdr["magic"]) != SNAP_MAGIC:
        raise DtrlError("not a snapshot blob (magic)")
    n = int(hdr["n_envs"]); off = int(hdr["header_bytes"])
    ids = raw[off:off + 4 * n].view(np.int32)
    off += (4 * n + 7) & ~7
    dt = env_state_dtype(np.float32 if int(hdr["sizeof_real"]) == 4 else np.float64)
    if dt.itemsize != int(hdr["sizeof_env_state"]):
        raise DtrlError("env_state dtype is %d bytes, the blob's EnvState %d" % (dt.itemsize, int(hdr["sizeof_env_state"])))
    eb = int(hdr["env_bytes"])
    st = np.ndarray((n,), dt, buffer=blob, offset=off, strides=(eb,))
    return hdr, ids, st


class BatchScenario:
    """N reference-shaped scenarios (cScenarioExp / cScenarioPoliEval / cScenarioSimChar) stepped as one batch on one GPU."""

    def _library(self):
        """The HIP library; there is no other backend in the product (tests of the host logic subclass this from tests/conftest.py). `-physics_precision= f32`
        (extra_args) selects the fp32 build of the same source; the library itself refuses a precision it was not built for."""
        return _bind(LIB_PATH_F32 if self._precision == "f32" else LIB_PATH)

    def __init__(self, arg_file=None, num_envs=1, data_root=None, device_id=-1, extra_args=None):
        self._precision = str((extra_args or {}).get("physics_precision", "f64"))
        self._lib = self._library()
        _warn_hw_queues()
        argv = []
        if extra_args:
            for k, v in extra_args.items():
                argv += ["-%s=" % k, str(v)]
        if data_root is not None:
            argv += ["-data_root=", str(data_root)]
        if arg_file is not None:
            argv += ["-arg_file=", str(arg_file)]
        self._argv = list(argv)
        self._device_id = int(device_id)
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        h = C.c_void_p()
        rc = self._lib.dtrl_create(arr, len(argv), int(num_envs), int(device_id), C.byref(h))
        if rc != DTRL_OK:
            raise DtrlError("dtrl_create failed (%d): %s" % (rc, self._lib.dtrl_last_error(None).decode()))
        self._h = h
        self.num_envs = int(num_envs)
        d = [C.c_int() for _ in range(8)]
        self._lib.dtrl_dims(self._h, *[C.byref(x) for x in d])
        self.L, self.D, self.S, self.A, self.P, self.nn_out, self.num_frags, self.frag_size = (x.value for x in d)
        self.W = 1 + 2 * self.S + self.A
        d = [C.c_int() for _ in range(4)]
        self._lib.dtrl_action_dims(self._h, *[C.byref(x) for x in d])
        self.n_opt, self.n_labels, self.num_update_steps, ext = (x.value for x in d)
        self.external = bool(ext)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dtrl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != DTRL_OK:
            raise DtrlError("dtrl call failed (%d): %s" % (rc, self._lib.dtrl_last_error(self._h).decode()))

    def _ids(self, env_ids):
        if env_ids is None:
            return None, self.num_envs
        a = np.ascontiguousarray(env_ids, np.int32)
        return a, len(a)

    def _assign_keys(self, fn, who, noun, env_ids, keys, *more):   # the ctypes marshalling policy slots, model variants and terrain sets share; fn: the family's entry point
        ka = np.ascontiguousarray(keys, np.int32)
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        if ids is not None and ids.shape != ka.shape:
            raise DtrlError("%s: env_ids and %s must have the same length" % (who, noun))
        self._chk(fn(self._h, _p(ids), len(ka), _p(ka), *more))

    def _get_keys(self, fn, env_ids):
        ids, n = self._ids(env_ids)
        out = np.zeros(n, np.int32)
        self._chk(fn(self._h, _p(ids), n, _p(out)))
        return out

    def _key_stats(self, fn, key):
        a = C.c_double(); n, e, c, r = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(fn(self._h, int(key), C.byref(n), C.byref(a), C.byref(e), C.byref(c), C.byref(r)))
        return {"n_envs": n.value, "avg_dist": a.value, "episodes": e.value, "cycles": c.value, "resets": r.value}

    # ---- cScenario interface ----
    def Update(self, dt=1.0 / 30.0):
        self._chk(self._lib.dtrl_step(self._h, float(dt)))

    def UpdateBegin(self, dt=1.0 / 30.0):
        """Queue one outer frame on the engine's stream and return (dtrl_step_begin); pair with UpdateEnd()."""
        self._chk(self._lib.dtrl_step_begin(self._h, dt))

    def UpdateEnd(self):
        self._chk(self._lib.dtrl_step_end(self._h))

    def UpdateEndBegin(self, dt=1.0 / 30.0):
        """UpdateEnd() + UpdateBegin(dt) without the barrier between them (dtrl_step_end_begin): each env group is relaunched as soon as its own frame is done."""
        self._chk(self._lib.dtrl_step_end_begin(self._h, float(dt)))

    def UpdatePoll(self, dt=1.0 / 30.0):
        """dtrl_step_poll: relaunch, without blocking, every env group whose frame has already ended (between two UpdateEndBegin calls, after the drain).
        Returns how many groups were relaunched."""
        n = C.c_int(0)
        self._chk(self._lib.dtrl_step_poll(self._h, float(dt), C.byref(n)))
        return n.value

    # ---- external policy mode (extra_args={"policy_mode": "external"}; include/dtrl.h) ----
    def PendingActions(self, with_states=True):
        """(ids int32[m], states float64[m][S]) of the envs parked at a decision, ascending env id (dtrl_pending_actions). After Update(), hand the states to
        your policy and give every env its row with SupplyActions; the next Update() carries them on."""
        ids = np.empty(self.num_envs, np.int32)
        st = np.empty((self.num_envs, self.S), np.float64) if with_states else None
        n = C.c_int(0)
        self._chk(self._lib.dtrl_pending_actions(self._h, _p(ids), _p(st), self.num_envs, C.byref(n)))
        return ids[:n.value].copy(), (st[:n.value].copy() if with_states else None)

    def SupplyActions(self, ids, action_ids, params, flags=None):
        """One action row per awaiting env (dtrl_supply_actions): action_ids int[m] (labels, 0 .. n_labels - 1; None = zeros), params float64[m][n_opt], flags uint32[m]
        (TUPLE_EXP_CRITIC | TUPLE_EXP_ACTOR; None = zeros). All or nothing: raises DtrlError if any listed env is not awaiting."""
        ids = np.ascontiguousarray(ids, np.int32)
        prm = np.ascontiguousarray(params, np.float64).reshape(len(ids), self.n_opt) if len(ids) else np.zeros((0, self.n_opt))
        aid = None if action_ids is None else np.ascontiguousarray(action_ids, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        if (aid is not None and len(aid) != len(ids)) or (fl is not None and len(fl) != len(ids)):
            raise DtrlError("SupplyActions: action_ids / flags must have one entry per env id")
        self._chk(self._lib.dtrl_supply_actions(self._h, _p(ids), len(ids), _p(aid), _p(prm), _p(fl)))

    def PendingActionsDevice(self, env_ids_ptr, states_ptr, cap):
        """dtrl_pending_actions_device on raw device pointers (int32[cap], float32[cap][S]); returns the number of awaiting envs written."""
        n = C.c_int(0)
        self._chk(self._lib.dtrl_pending_actions_device(self._h, C.c_void_p(env_ids_ptr), C.c_void_p(states_ptr) if states_ptr else None, int(cap), C.byref(n)))
        return n.value

    def SupplyActionsDevice(self, env_ids_ptr, n, action_ids_ptr, params_ptr, flags_ptr=None):
        """dtrl_supply_actions_device on raw device pointers (int32[n], int32[n] or 0, float32[n][n_opt], uint32[n] or 0); returns the number of rejected rows."""
        rej = C.c_int(0)
        self._chk(self._lib.dtrl_supply_actions_device(self._h, C.c_void_p(env_ids_ptr), int(n), C.c_void_p(action_ids_ptr) if action_ids_ptr else None,
                                                       C.c_void_p(params_ptr), C.c_void_p(flags_ptr) if flags_ptr else None, C.byref(rej)))
        return rej.value

    def ExtStats(self):
        """dict(awaiting, ready, env_steps_total, env_frames_total): envs parked without / with a delivered action, env-steps and env frames run since creation."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(self._lib.dtrl_ext_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("awaiting", "ready", "env_steps_total", "env_frames_total"), (x.value for x in v)))

    def ExtEnvInfo(self, env_ids=None):
        """(park int32[n]: 0 running / frame complete, 1 awaiting, 2 action delivered; steps_left int32[n]: env-steps the env's current frame has yet to finish)"""
        ids, n = self._ids(env_ids)
        park = np.zeros(n, np.int32); left = np.zeros(n, np.int32)
        self._chk(self._lib.dtrl_ext_env_info(self._h, _p(ids), n, _p(park), _p(left)))
        return park, left

    def ExtLaunchMs(self, which):
        """Device time (ms) of the collection (0) / scatter (1) launches since the last call."""
        return float(self._lib.dtrl_ext_launch_ms(self._h, int(which)))

    def StepUpdates(self, n):
        self._chk(self._lib.dtrl_step_updates(self._h, int(n)))

    def RunFrames(self, frames, dt=1.0 / 30.0):
        self._chk(self._lib.dtrl_run_frames(self._h, int(frames), float(dt)))

    def Reset(self, env_ids=None, terrain_seeds=None):
        ids, n = self._ids(env_ids)
        seeds = None if terrain_seeds is None else np.ascontiguousarray(terrain_seeds, np.uint64)
        self._chk(self._lib.dtrl_reset(self._h, _p(ids), n, _p(seeds)))

    def SetPolicy(self, weights, in_off=None, in_scale=None, out_off=None, out_scale=None):
        w = np.ascontiguousarray(weights, np.float32)
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (in_off, in_scale, out_off, out_scale)]
        self._chk(self._lib.dtrl_set_policy(self._h, _p(w), w.size, *[_p(a) for a in arrs]))
        self._policy = (w.copy(), arrs[0], arrs[1])     # kept for the NN-activation recorder (recorders.py)

    def PolicyNumParams(self):
        n = C.c_size_t()
        self._chk(self._lib.dtrl_policy_num_params(self._h, C.byref(n)))
        return n.value

    def BuildNNOutputOffsetScale(self):
        off = np.zeros(self.nn_out); sc = np.zeros(self.nn_out)
        self._chk(self._lib.dtrl_build_output_offset_scale(self._h, _p(off), _p(sc)))
        return off, sc

    def LoadModel(self, model_file):
        """cNeuralNet::LoadModel (learning/NeuralNet.cpp:110-135): Caffe HDF5 weights by layer name, then the normalisers from
        '<model>_scale.txt' next to it when that file exists (GetOffsetScaleFile)."""
        from . import caffe_hdf5
        w = caffe_hdf5.load_mace_weights(model_file, self.num_frags)
        if w.size != self.PolicyNumParams():
            raise DtrlError("%s holds %d parameters, the deploy net needs %d" % (model_file, w.size, self.PolicyNumParams()))
        self.SetPolicy(w)
        scale = os.path.splitext(model_file)[0] + "_scale.txt"
        if os.path.exists(scale):
            self.LoadScale(scale)
        return w

    def LoadScale(self, path):
        """cNeuralNet::LoadScale: install the normaliser vectors of a '<model>_scale.txt' file (weights untouched)."""
        self._chk(self._lib.dtrl_load_scale_file(self._h, os.fsencode(path)))

    def WriteOffsetScale(self, path):
        """cNeuralNet::WriteOffsetScale: write the current normalisers in the reference's file format."""
        self._chk(self._lib.dtrl_write_scale_file(self._h, os.fsencode(path)))

    def SetExplore(self, enable, rate, temp, base_rate):
        self._chk(self._lib.dtrl_set_explore(self._h, int(enable), float(rate), float(temp), float(base_rate)))

    def SetTerrainParamsLerp(self, lerp):
        self._chk(self._lib.dtrl_set_terrain_lerp(self._h, float(lerp)))

    def DrainTuples(self, cap=None):
        cap = cap or max(2 * self.num_envs, 64)
        buf = getattr(self, "_drain_buf", None)
        if buf is None or buf[0].shape[0] < cap:     # (20 MB at 4096 envs: kept, not allocated and zero-filled per call)
            buf = self._drain_buf = (np.empty((cap, self.W), np.float32), np.empty(cap, np.uint32), np.empty(cap, np.int32))
        rows, fl, ids = buf
        n = C.c_int()
        self._chk(self._lib.dtrl_drain_tuples(self._h, _p(rows), _p(fl), _p(ids), cap, C.byref(n)))
        return rows[:n.value].copy(), fl[:n.value].copy(), ids[:n.value].copy()

    def DrainTuplesDevice(self, rows_ptr, flags_ptr, ids_ptr, cap):
        """dtrl_drain_tuples_device: raw DEVICE pointers (e.g. tensor.data_ptr()) of float32 [cap, W] / uint32 [cap] / int32 [cap]; returns n."""
        n = C.c_int()
        self._chk(self._lib.dtrl_drain_tuples_device(self._h, C.c_void_p(rows_ptr), C.c_void_p(flags_ptr) if flags_ptr else None, C.c_void_p(ids_ptr) if ids_ptr else None, int(cap), C.byref(n)))
        return n.value

    def DrainTuplesPacked(self, block_ptr, block_rows, want_count=False):
        """Pending tuples -> ONE device block [block_rows + 1, W + 2] float32 (header row, then rows sorted by env id with the flag word and the GLOBAL
        env id as int32 bit patterns in the two extra columns); the ring is emptied. Returns the row count when want_count (a 4-byte read-back), else None."""
        n = C.c_int(0)
        self._chk(self._lib.dtrl_drain_tuples_packed(self._h, C.c_void_p(int(block_ptr)), int(block_rows), C.byref(n) if want_count else None))
        return n.value if want_count else None

    def TupleStats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64(); cap = C.c_int32()
        self._chk(self._lib.dtrl_tuple_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(cap)))
        return {"pending": a.value, "drained": b.value, "dropped": c.value, "capacity": cap.value}

    def SetPolicyDevice(self, weights_ptr, n, in_off_ptr=None, in_scale_ptr=None, out_off_ptr=None, out_scale_ptr=None):
        """dtrl_set_policy_device: raw DEVICE pointers (float32 weights in Caffe blob order, float64 normalisers or None)."""
        q = [C.c_void_p(x) if x else None for x in (in_off_ptr, in_scale_ptr, out_off_ptr, out_scale_ptr)]
        self._chk(self._lib.dtrl_set_policy_device(self._h, C.c_void_p(weights_ptr), int(n), *q))

    def SetPolicyDeviceOn(self, weights_ptr, n, stream_ptr):
        """dtrl_set_policy_device_on: weights only, the re-layout kernel on the caller's stream (hipStream_t as an int), returns when it has run."""
        self._chk(self._lib.dtrl_set_policy_device_on(self._h, C.c_void_p(weights_ptr), int(n), C.c_void_p(int(stream_ptr)) if stream_ptr else None))

    def SetPolicyDeviceAsync(self, weights_ptr, n, stream_ptr):
        """dtrl_set_policy_device_async: weights only, the re-layout kernel queued on the caller's stream, NO host wait; every env's next launch waits for it on the device."""
        self._chk(self._lib.dtrl_set_policy_device_async(self._h, C.c_void_p(weights_ptr), int(n), C.c_void_p(int(stream_ptr)) if stream_ptr else None))

    def GetDistLog(self):
        """cScenarioPoliEval::GetDistLog over the batch: (distances, env ids), grouped by env, episodes in time order."""
        n = C.c_int()
        self._chk(self._lib.dtrl_get_dist_log(self._h, None, None, 0, C.byref(n)))
        d = np.zeros(n.value); ids = np.zeros(n.value, np.int32)
        if n.value:
            self._chk(self._lib.dtrl_get_dist_log(self._h, _p(d), _p(ids), n.value, C.byref(n)))
        return d, ids

    def ResetAvgDist(self):
        self._chk(self._lib.dtrl_reset_avg_dist(self._h))

    def OutputResults(self, out_file):
        """cOptScenarioPoliEval::OutputResults: append the dist log as one line to out_file."""
        self._chk(self._lib.dtrl_write_dist_log(self._h, os.fsencode(out_file)))

    # ---- character / controller observability ----
    def PoseVel(self, env_ids=None):
        ids, n = self._ids(env_ids)
        q = np.zeros((n, self.D)); qd = np.zeros((n, self.D))
        self._chk(self._lib.dtrl_get_pose_vel(self._h, _p(ids), n, _p(q), _p(qd)))
        return q, qd

    def BuildPose(self, env_ids=None):
        return self.PoseVel(env_ids)[0]

    def BuildVel(self, env_ids=None):
        return self.PoseVel(env_ids)[1]

    def LinkStates(self, env_ids=None):
        """World COM position [n, L, 2], COM velocity [n, L, 2] and body angle [n, L] of every link (GetBodyPart(i)->GetPos() ...)."""
        ids, n = self._ids(env_ids)
        c = np.zeros((n, self.L, 2)); v = np.zeros((n, self.L, 2)); a = np.zeros((n, self.L))
        self._chk(self._lib.dtrl_get_link_states(self._h, _p(ids), n, _p(c), _p(v), _p(a)))
        return c, v, a

    def AddPerturb(self, link, force, duration, local_pos=None, env_ids=None):
        """cScenarioSimChar::AddPerturb with an ePerturbForce: world-frame force [n, 2] on body part link [n] for duration [n] seconds."""
        ids, n = self._ids(env_ids)
        link = np.ascontiguousarray(np.broadcast_to(np.asarray(link, np.int32), (n,)))
        force = np.ascontiguousarray(np.broadcast_to(np.asarray(force, np.float64), (n, 2)))
        duration = np.ascontiguousarray(np.broadcast_to(np.asarray(duration, np.float64), (n,)))
        lp = None if local_pos is None else np.ascontiguousarray(np.broadcast_to(np.asarray(local_pos, np.float64), (n, 2)))
        self._chk(self._lib.dtrl_add_perturb(self._h, _p(ids), n, _p(link), _p(lp) if lp is not None else None, _p(force), _p(duration)))

    def ApplyRandForce(self, seed=0, env_ids=None):
        """cScenarioSimChar::ApplyRandForce(): random body part / direction / magnitude / duration per env."""
        ids, n = self._ids(env_ids)
        self._chk(self._lib.dtrl_apply_rand_force(self._h, _p(ids), n, int(seed)))

    # ---- push schedule: random pushes on the device at per-env random times (the reference calls ApplyRandForce by hand) ----
    def PushSchedule(self, wait, seed=0, force=None, duration=None):
        """dtrl_push_schedule: from now on every env of scale != 0 is pushed at random times -- wait = (lo, hi) frame boundaries between two pushes of an env
        (1 <= lo <= hi), force = (lo, hi) magnitude range, duration = (lo, hi) seconds; None: the batch's -min_perturb= ... arguments. Link, direction, magnitude
        and duration are drawn as ApplyRandForce draws them, from a stream of (seed, global env id, the env's own counter) alone, and written into the env's
        perturbation slot at its frame boundary by one small launch per env group (no host wait). An episode start draws a new wait and never pushes.
        PushSchedule((1, 0)) removes the schedule (records, counters and scales stay). Not with -policy_mode= external."""
        nan = float("nan")
        f = (nan, nan) if force is None else force
        d = (nan, nan) if duration is None else duration
        self._chk(self._lib.dtrl_push_schedule(self._h, int(wait[0]), int(wait[1]), int(seed) & 0xFFFFFFFFFFFFFFFF, float(f[0]), float(f[1]), float(d[0]), float(d[1])))

    def PushScale(self, scales, env_ids=None):
        """dtrl_push_scale: per-env factor on the scheduled force (finite, >= 0; 1.0 unless set). 0 takes the env out of the schedule."""
        ids, n = self._ids(env_ids)
        scales = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, np.float64), (n,)))
        self._chk(self._lib.dtrl_push_scale(self._h, _p(ids), n, _p(scales)))

    def PushInfo(self, env_ids=None):
        """dtrl_push_info: {"wait", "pushes", "last_link" (int32 per listed env, all by default; last_link -1: none yet), "last_force" [n, 2], "last_dur" [n]}."""
        ids, n = self._ids(env_ids)
        wait, pushes, link = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        force, dur = np.zeros((n, 2), np.float64), np.zeros(n, np.float64)
        self._chk(self._lib.dtrl_push_info(self._h, _p(ids), n, _p(wait), _p(pushes), _p(link), _p(force), _p(dur)))
        return {"wait": wait, "pushes": pushes, "last_link": link, "last_force": force, "last_dur": dur}

    # ---- episode limits: episodes end by time or distance on the device (the reference's end by a fall alone) ----
    def EpisodeLimit(self, frames=None, dist=None, seed=0):
        """dtrl_episode_limit: from now on an env's episode ends -- as if the env had fallen, without a FAIL tuple -- after a number of frame boundaries drawn per
        episode from frames = (lo, hi) (1 <= lo <= hi; None: no frame limit), or once its root is dist past the spawn x (None: no distance limit). The draw is a
        function of (seed, global env id, the env's draws so far). One small launch per env group and frame, no host wait. EpisodeLimit() removes the limit
        (records, counters and flags stay). Not with -policy_mode= external."""
        lo, hi = (0, 0) if frames is None else frames
        self._chk(self._lib.dtrl_episode_limit(self._h, int(lo), int(hi), float("inf") if dist is None else float(dist), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def EpisodeLimitEnvs(self, on, env_ids=None):
        """dtrl_episode_limit_envs: per-env flag (1 unless set); 0 holds the env out of the limit: its episodes end by a fall alone and its record stays as it is."""
        ids, n = self._ids(env_ids)
        on = np.ascontiguousarray(np.broadcast_to(np.asarray(on).astype(bool).astype(np.uint8), (n,)))
        self._chk(self._lib.dtrl_episode_limit_envs(self._h, _p(ids), n, _p(on)))

    def EpisodeInfo(self, env_ids=None):
        """dtrl_episode_info: {"frames", "limit", "last_frames", "last_cause" (int32 per listed env, all by default; cause 1 fall, 2 frame limit, 3 distance, 0 none
        yet), "by_fall", "by_limit" (int64), "last_dist" (float64)} as of the last completed boundary."""
        ids, n = self._ids(env_ids)
        out = {k: np.zeros(n, t) for k, t in (("frames", np.int32), ("limit", np.int32), ("by_fall", np.int64), ("by_limit", np.int64), ("last_frames", np.int32),
                                              ("last_dist", np.float64), ("last_cause", np.int32))}
        self._chk(self._lib.dtrl_episode_info(self._h, _p(ids), n, *[_p(v) for v in out.values()]))
        return out

    # ---- frame trace: per-frame state rows of chosen envs, recorded on the device (the reference writes cCharacter::WriteState per frame, or shows the GUI) ----
    def Trace(self, env_ids=None, frames=300):
        """dtrl_trace: from now on every listed env (distinct local ids in any order; None: every env) writes one compact row per frame boundary into its own ring
        of `frames` rows in device memory -- behind the frame and the episode limit, in front of everything that resets an env, so a row holds the pose the frame
        ended in (a fallen one included), the need_reset the later rules see and the keys the frame ran under. One small launch per env group and frame, no host
        wait. A second call replaces the trace (counters from 0); Trace(None, 0) or TraceOff() removes it."""
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        n = 0 if int(frames) == 0 and ids is None else (self.num_envs if ids is None else len(ids))
        self._chk(self._lib.dtrl_trace(self._h, _p(ids), n, int(frames)))

    def TraceOff(self):
        self._chk(self._lib.dtrl_trace(self._h, None, 0, 0))

    def TraceInfo(self):
        """dtrl_trace_info: {"n_traced", "frames", "width" (3 D + 2), "env_ids" (int32, Trace's order), "rows_written" (int64 per traced env)}."""
        n, f, w = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._lib.dtrl_trace_info(self._h, C.byref(n), C.byref(f), C.byref(w), None, None))
        ids, rows = np.zeros(n.value, np.int32), np.zeros(n.value, np.int64)
        if n.value:
            self._chk(self._lib.dtrl_trace_info(self._h, None, None, None, _p(ids), _p(rows)))
        return {"n_traced": n.value, "frames": f.value, "width": w.value, "env_ids": ids, "rows_written": rows}

    TRACE_INTS = ("row", "need_reset", "action_id", "state", "stance", "contact_bits", "num_cycles", "num_resets", "slot", "variant", "terrain", "reserved")

    def _trace_shape(self, env_ids, max_rows):
        info = self.TraceInfo()
        ids = info["env_ids"] if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        rows = min(info["frames"], int(info["rows_written"].max()) if info["n_traced"] else 0) if max_rows is None else int(max_rows)
        return ids, rows, info["width"]

    def TraceRead(self, env_ids=None, max_rows=None):
        """dtrl_trace_read: the last count[i] = min(rows written, frames, max_rows) rows of each listed traced env (None: all, in Trace's order), oldest first, as a
        dict of arrays [n, max_rows, ...]: "time", "phase", "q", "qd", "tau" (float64), "row", "need_reset", "action_id", "state", "stance", "contact_bits",
        "num_cycles", "num_resets", "slot", "variant", "terrain" (int32), plus "count" [n], "env_ids" [n] and the raw blocks "vals" / "ints". Rows beyond count[i]
        are zero. max_rows None: as many rows as the fullest ring holds."""
        ids, rows, W = self._trace_shape(env_ids, max_rows)
        n, D = len(ids), self.D
        vals, ints, count = np.zeros((n, rows, W), np.float64), np.zeros((n, rows, 12), np.int32), np.zeros(n, np.int32)
        self._chk(self._lib.dtrl_trace_read(self._h, _p(ids), n, rows, _p(vals), _p(ints), _p(count)))
        out = {"time": vals[:, :, 0], "phase": vals[:, :, 1], "q": vals[:, :, 2:2 + D], "qd": vals[:, :, 2 + D:2 + 2 * D], "tau": vals[:, :, 2 + 2 * D:2 + 3 * D]}
        out.update({k: ints[:, :, i] for i, k in enumerate(self.TRACE_INTS) if k != "reserved"})
        out.update({"count": count, "env_ids": ids, "vals": vals, "ints": ints})
        return out

    def TraceReadDevice(self, env_ids=None, max_rows=None):
        """dtrl_trace_read_device: the same rows into two torch tensors on the batch's device -- (vals [n, max_rows, W] float64, ints [n, max_rows, 12] int32) -- and
        count [n] as a numpy array; one launch, nothing but the counts crosses to the host."""
        import torch
        ids, rows, W = self._trace_shape(env_ids, max_rows)
        n = len(ids)
        dev = torch.device("cuda", self._device_id if self._device_id >= 0 else torch.cuda.current_device())
        vals = torch.zeros((n, rows, W), dtype=torch.float64, device=dev); ints = torch.zeros((n, rows, 12), dtype=torch.int32, device=dev)
        count = np.zeros(n, np.int32)
        torch.cuda.synchronize(dev)   # (the zero fills run on torch's stream, the gather on the batch's)
        self._chk(self._lib.dtrl_trace_read_device(self._h, _p(ids), n, rows, C.c_void_p(vals.data_ptr()), C.c_void_p(ints.data_ptr()), _p(count)))
        return vals, ints, count

    # ---- episode log: one row per ended episode, recorded on the device (the reference logs one distance per episode: cScenarioPoliEval::RecordDistTraveled) ----
    def EpisodeLog(self, capacity):
        """dtrl_episode_log: from now on every ended episode appends one 64-byte row to a ring of `capacity` rows per env group in page-locked host memory, written
        on the device at the frame boundary behind the episode limit and the trace and in front of every rule that moves a key or redraws a scale: how long the
        episode lasted, how far it got, why it ended and under which slot, variant, terrain and rescale draw it ran. One launch of one workgroup per env group and
        frame, no host wait. A second call replaces the log (everything from 0); EpisodeLog(0) or EpisodeLogOff() removes it."""
        self._chk(self._lib.dtrl_episode_log(self._h, int(capacity)))

    def EpisodeLogOff(self):
        self._chk(self._lib.dtrl_episode_log(self._h, 0))

    def EpisodeLogInfo(self):
        """dtrl_episode_log_info: {"capacity" (rows per ring, 0: no log), "n_groups", "written" (rows ever appended), "lost" (rows overwritten before a drain took them)}."""
        cap, g, w, lost = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self._lib.dtrl_episode_log_info(self._h, C.byref(cap), C.byref(g), C.byref(w), C.byref(lost)))
        return {"capacity": cap.value, "n_groups": g.value, "written": w.value, "lost": lost.value}

    def EpisodeLogDrain(self, max_rows=None):
        """dtrl_episode_log_drain: the rows not drained yet, merged over the env groups in (boundary, env) order, as a dict of numpy arrays, one per field of
        EPISODE_ROW_DTYPE ("env", "cause" 1 fall / 2 frame limit / 3 distance, "frames", "cycles", "boundary", "episode", "dist", "need_reset", "slot", "variant",
        "terrain", "rescale_draw"), plus "lost": rows this call found overwritten before it could take them. max_rows None: all of them. Never queues GPU work;
        between UpdateBegin and UpdateEnd it does not wait and returns what has been published so far, otherwise it waits for queued work first."""
        parts, lost_total = [], 0
        left = None if max_rows is None else int(max_rows)
        while left is None or left > 0:
            cap = 4096 if left is None else min(left, 4096)
            rows, n, lost = np.zeros(cap, EPISODE_ROW_DTYPE), C.c_int32(), C.c_int64()
            self._chk(self._lib.dtrl_episode_log_drain(self._h, _p(rows), cap, C.byref(n), C.byref(lost)))
            lost_total += lost.value
            parts.append(rows[:n.value])
            if left is not None:
                left -= n.value
            if n.value < cap:
                break
        rows = np.concatenate(parts) if parts else np.zeros(0, EPISODE_ROW_DTYPE)
        out = {k: np.ascontiguousarray(rows[k]) for k in EPISODE_ROW_DTYPE.names if k != "zero"}
        out["lost"] = lost_total
        return out

    def VariantRescaleFactors(self, env_ids, draws):
        """dtrl_variant_rescale_factors: factors [n, 4, L] in RESCALE_QUANTITIES order that env env_ids[i] drew for its draw number draws[i] -- a row's
        "rescale_draw" --, by the library's rule on the host; draw -1 gives all 1. What VariantRescaleInfo()["factors"] shows for the current episode alone."""
        ids, dr = np.ascontiguousarray(env_ids, np.int32), np.ascontiguousarray(draws, np.int32)
        if ids.shape != dr.shape or ids.ndim != 1:
            raise DtrlError("VariantRescaleFactors: env_ids and draws must be two lists of the same length")
        out = np.zeros((len(ids), 4, self.L), np.float64)
        self._chk(self._lib.dtrl_variant_rescale_factors(self._h, _p(ids), _p(dr), len(ids), _p(out)))
        return out

    def SetPoseVel(self, q, qd, env_ids=None):
        ids, n = self._ids(env_ids)
        q = np.ascontiguousarray(q, np.float64).reshape(n, self.D); qd = np.ascontiguousarray(qd, np.float64).reshape(n, self.D)
        self._chk(self._lib.dtrl_set_pose_vel(self._h, _p(ids), n, _p(q), _p(qd)))

    def ContactCache(self, env_ids=None):
        """The persistent contact points of Bullet's manifolds (dtrl_get_contact_cache): (count[n], ids[n, 24], lambda[n, 24]) -- with (q, qd) the whole dynamic state."""
        ids, n = self._ids(env_ids)
        cnt = np.zeros(n, np.int32); rid = np.zeros((n, 24), np.int32); lam = np.zeros((n, 24))
        self._chk(self._lib.dtrl_get_contact_cache(self._h, _p(ids), n, _p(cnt), _p(rid), _p(lam)))
        return cnt, rid, lam

    def SetContactCache(self, count, row_ids, lam, env_ids=None):
        ids, n = self._ids(env_ids)
        cnt = np.ascontiguousarray(count, np.int32).reshape(n); rid = np.ascontiguousarray(row_ids, np.int32).reshape(n, 24); lam = np.ascontiguousarray(lam, np.float64).reshape(n, 24)
        self._chk(self._lib.dtrl_set_contact_cache(self._h, _p(ids), n, _p(cnt), _p(rid), _p(lam)))

    def SideStream(self, k=0):
        """(hipStream_t as an int, start delay in us measured at creation) of the k-th side stream: kernels queued there start on the compute units
        `reserve_cus` keeps out of the frame launches, while a frame is in flight. (None, -1.0) without a reservation."""
        d = C.c_double(-1.0)
        p = self._lib.dtrl_side_stream(self._h, int(k), C.byref(d))
        return (int(p) if p else None), float(d.value)

    def CommandAction(self, action_id, env_ids=None):
        """cCharController::CommandAction on the listed envs (all by default): action_id (an int, or one per env) is taken at the next cycle."""
        ids, n = self._ids(env_ids)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action_id, np.int32), (n,)))
        self._chk(self._lib.dtrl_command_action(self._h, _p(ids), n, _p(a)))

    def RecordPoliState(self, env_ids=None):
        ids, n = self._ids(env_ids)
        s = np.zeros((n, self.S))
        self._chk(self._lib.dtrl_get_poli_state(self._h, _p(ids), n, _p(s)))
        return s

    def SetTuplePipelining(self, on=True):
        """Two tuple rings, switched by every UpdateBegin: UpdateEnd(f); UpdateBegin(f + 1); DrainTuplesPacked(...) hands out frame f's tuples while
        frame f + 1 runs (the batched form of the reference's env threads feeding the trainer while the others keep stepping, scenarios/ScenarioTrain.cpp:376-410)."""
        self._chk(self._lib.dtrl_set_tuple_pipelining(self._h, 1 if on else 0))

    def PolicyOutput(self, env_ids=None):
        """cNeuralNet::GetLayerState("output") after the controller's last Eval, un-normalised like Eval's out_y (learning/NeuralNet.cpp:352-375, 814-834)."""
        ids, n = self._ids(env_ids)
        y = np.zeros((n, self.nn_out))
        self._chk(self._lib.dtrl_get_policy_output(self._h, _p(ids), n, _p(y)))
        return y

    def Flags(self, env_ids=None):
        ids, n = self._ids(env_ids)
        f = np.zeros(n, np.uint32)
        self._chk(self._lib.dtrl_get_flags(self._h, _p(ids), n, _p(f)))
        return f

    def Torques(self, env_ids=None):
        ids, n = self._ids(env_ids)
        a = np.zeros((n, self.D)); b = np.zeros((n, self.D))
        self._chk(self._lib.dtrl_get_torques(self._h, _p(ids), n, _p(a), _p(b)))
        return a, b

    def Contacts(self, env_ids=None):
        ids, n = self._ids(env_ids)
        f = np.zeros((n, self.L), np.int32)
        self._chk(self._lib.dtrl_get_contacts(self._h, _p(ids), n, _p(f)))
        return f

    def Ctrl(self, env_ids=None):
        ids, n = self._ids(env_ids)
        st = np.zeros(n, np.int32); ph = np.zeros(n); aid = np.zeros(n, np.int32); prm = np.zeros((n, self.P)); tg = np.zeros((n, self.L))
        self._chk(self._lib.dtrl_get_ctrl(self._h, _p(ids), n, _p(st), _p(ph), _p(aid), _p(prm), _p(tg)))
        return st, ph, aid, prm, tg

    def CycleInfo(self, env_ids=None):
        """Per env: cycle counter, reset counter, COM [n, 2] and simulated time at the start of the current cycle, optimisable params of the current action [n, frag_size]."""
        ids, n = self._ids(env_ids)
        nc = np.zeros(n, np.int64); nr = np.zeros(n, np.int64); com = np.zeros((n, 2)); t = np.zeros(n); prm = np.zeros((n, self.frag_size))
        self._chk(self._lib.dtrl_get_cycle_info(self._h, _p(ids), n, _p(nc), _p(nr), _p(com), _p(t), _p(prm)))
        return nc, nr, com, t, prm

    def ActionTable(self):
        """cTerrainRLCharController::BuildActionOptParams for every action: [n_actions, frag_size]."""
        na = C.c_int(0)
        self._chk(self._lib.dtrl_get_action_table(self._h, C.byref(na), None))
        tab = np.zeros((na.value, self.frag_size))
        self._chk(self._lib.dtrl_get_action_table(self._h, C.byref(na), _p(tab)))
        return tab

    def SampleGround(self, env, xs):
        xs = np.ascontiguousarray(xs, np.float64); n = len(xs)
        h = np.zeros(n); seg = np.zeros(n, np.int32); i = np.zeros(n, np.int32); j = np.zeros(n, np.int32)
        self._chk(self._lib.dtrl_sample_ground(self._h, int(env), n, _p(xs), _p(h), _p(seg), _p(i), _p(j)))
        return h, seg, i, j

    def GroundWindow(self, env):
        """One env's two-segment ground window in logical order: [(min_x, max_x, heights float32[w])] * 2 and the number of segments built so far
        (-1 unless -terrain_gen= device)."""
        w = (C.c_int32 * 2)(); mn = (C.c_double * 2)(); mx = (C.c_double * 2)(); nb = C.c_int64(0)
        h0 = np.zeros(512, np.float32); h1 = np.zeros(512, np.float32)
        self._chk(self._lib.dtrl_get_ground_window(self._h, int(env), w, mn, mx, _p(h0), _p(h1), 512, C.byref(nb)))
        return [(mn[0], mx[0], h0[:w[0]].copy()), (mn[1], mx[1], h1[:w[1]].copy())], nb.value

    def EvalStats(self):
        a = C.c_double(); e, c, r = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._lib.dtrl_eval_stats(self._h, C.byref(a), C.byref(e), C.byref(c), C.byref(r)))
        return {"avg_dist": a.value, "episodes": e.value, "cycles": c.value, "resets": r.value}

    # ---- policy slots: several policies in one batch, one per env (no counterpart in the reference: it keeps one net per scene object) ----
    def CreateSlots(self, n_slots):
        """dtrl_slots_create: 1 .. 32 slots, once per batch. Slot 0 is the batch's own policy (SetPolicy*, LoadScale, SetExplore keep acting on it); every env starts in it."""
        self._chk(self._lib.dtrl_slots_create(self._h, int(n_slots)))
        self.num_slots = int(n_slots)

    def SlotSetPolicy(self, slot, weights, in_off=None, in_scale=None, out_off=None, out_scale=None):
        """SetPolicy into a slot. `weights` is a host array (float32, Caffe blob order; normalisers float64 arrays, None = identity) or a torch tensor on the
        batch's GPU (float32; normalisers float64 device tensors, None = keep the slot's vector -- dtrl_slot_set_policy_device). Between frames only."""
        if hasattr(weights, "data_ptr") and getattr(weights, "is_cuda", False):
            ts = [weights] + [t for t in (in_off, in_scale, out_off, out_scale)]
            for t in ts:
                if t is not None and not (hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous()):
                    raise DtrlError("SlotSetPolicy: with device weights every normaliser must be a contiguous device tensor (or None)")
            if str(weights.dtype) != "torch.float32" or not weights.is_contiguous():
                raise DtrlError("SlotSetPolicy: device weights must be a contiguous float32 tensor")
            q = [None if t is None else C.c_void_p(t.data_ptr()) for t in ts[1:]]
            import torch
            torch.cuda.current_stream(weights.device).synchronize()      # the tensors are complete before the engine's stream reads them
            self._chk(self._lib.dtrl_slot_set_policy_device(self._h, int(slot), C.c_void_p(weights.data_ptr()), int(weights.numel()), *q))
            return
        w = np.ascontiguousarray(weights, np.float32)
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (in_off, in_scale, out_off, out_scale)]
        self._chk(self._lib.dtrl_slot_set_policy(self._h, int(slot), _p(w), w.size, *[_p(a) for a in arrs]))

    def SlotLoadModel(self, slot, model_file):
        """LoadModel into a slot: Caffe HDF5 weights by layer name plus the normalisers of '<model>_scale.txt' next to it when that file exists."""
        from . import caffe_hdf5
        w = caffe_hdf5.load_mace_weights(model_file, self.num_frags)
        if w.size != self.PolicyNumParams():
            raise DtrlError("%s holds %d parameters, the deploy net needs %d" % (model_file, w.size, self.PolicyNumParams()))
        scale = os.path.splitext(model_file)[0] + "_scale.txt"
        norm = (None,) * 4
        if os.path.exists(scale):
            import json
            with open(scale) as f:
                j = json.load(f)
            norm = tuple(None if j.get(k) is None else np.asarray(j[k], np.float64) for k in ("InputOffset", "InputScale", "OutputOffset", "OutputScale"))
        self.SlotSetPolicy(slot, w, *norm)
        return w

    def SlotAlias(self, slot, src_slot):
        """dtrl_slot_alias: `slot` reads src_slot's weights and normalisers from now on (hand-overs into slot 0 included) and keeps its own exploration settings."""
        self._chk(self._lib.dtrl_slot_alias(self._h, int(slot), int(src_slot)))

    def SlotSetExplore(self, slot, enable, rate, temp, base_rate):
        self._chk(self._lib.dtrl_slot_set_explore(self._h, int(slot), int(enable), float(rate), float(temp), float(base_rate)))

    def AssignSlots(self, env_ids, slots):
        """env_ids[i] -> slots[i] (env_ids None: the first len(slots) envs); takes effect with the env's next launch. Between frames only."""
        self._assign_keys(self._lib.dtrl_assign_slots, "AssignSlots", "slots", env_ids, slots)

    def GetSlots(self, env_ids=None):
        return self._get_keys(self._lib.dtrl_get_slots, env_ids)

    def SlotStats(self, slot):
        """EvalStats restricted to the envs currently in `slot` (plus their number), reduced on the device in a fixed order."""
        return self._key_stats(self._lib.dtrl_slot_stats, slot)

    # ---- model variants: several character models in one batch, one per env (no counterpart in the reference, which keeps one character per scene object) ----
    num_variants = 0

    def CreateVariants(self, n_variants):
        """dtrl_variants_create: a table of 1 .. num_envs complete character models, once per batch. Variant 0 is the batch's own model and every env starts in it;
        variants >= 1 are empty until LoadVariant / LoadVariantJson / ScaledVariant fills them. Not together with policy slots or external policy mode."""
        self._chk(self._lib.dtrl_variants_create(self._h, int(n_variants)))
        self.num_variants = int(n_variants)

    def LoadVariant(self, v, path):
        """dtrl_variant_load_file: variant v >= 1 from a character file (resolved like -character_file=), through the loader the batch was created with. Masses, box
        sizes, attach points, joint limits and PD settings may differ from the batch's model; skeleton, scene and controller part may not. Between frames only."""
        self._chk(self._lib.dtrl_variant_load_file(self._h, int(v), os.fsencode(str(path))))

    def LoadVariantJson(self, v, text):
        """dtrl_variant_load_json: the same from the character description itself (str or bytes)."""
        raw = text.encode() if isinstance(text, str) else bytes(text)
        self._chk(self._lib.dtrl_variant_load_json(self._h, int(v), raw, len(raw)))

    def CharacterFile(self):
        """The batch's character file as the library resolves it: -character_file= of the creation arguments, relative to -data_root= unless absolute."""
        vals = []
        for key in ("character_file", "data_root"):
            arr = (C.c_char_p * len(self._argv))(*[a.encode() for a in self._argv])
            buf = C.create_string_buffer(4096); found = C.c_int(); nt = C.c_int()
            rc = self._lib.dtrl_args_parse_string(arr, len(self._argv), key.encode(), buf, 4096, C.byref(found), C.byref(nt))
            if rc != DTRL_OK:
                raise DtrlError("dtrl_args_parse_string failed (%d): %s" % (rc, self._lib.dtrl_last_error(None).decode()))
            vals.append(buf.value.decode() if found.value else "")
        path, root = vals
        return path if (not path or path.startswith("/") or not root) else os.path.join(root, path)

    def ScaledVariant(self, v, mass=None, size=None, kp=1.0, kd=1.0, torque_lim=1.0):
        """Variant v = the batch's character with scaled bodies and motors, loaded through LoadVariantJson (no file is written). `mass` / `size`: one factor for
        every body, or {body name: factor} (BodyDefs[].Name; size scales the box's Param0 and Param1); kp / kd / torque_lim: one factor for every PD controller,
        or {joint name: factor} (PDControllers[].Name). Returns the JSON text that was loaded."""
        import json
        with open(self.CharacterFile()) as f:
            doc = json.load(f)

        def factor(spec, name):
            if spec is None:
                return 1.0
            if isinstance(spec, dict):
                return float(spec.get(name, 1.0))
            return float(spec)
        for spec, what in ((mass, "mass"), (size, "size")):
            if isinstance(spec, dict):
                unknown = set(spec) - {b.get("Name") for b in doc["BodyDefs"]}
                if unknown:
                    raise DtrlError("ScaledVariant: %s names no body of the character: %s" % (what, ", ".join(sorted(map(str, unknown)))))
        for b in doc["BodyDefs"]:
            b["Mass"] = b["Mass"] * factor(mass, b.get("Name"))
            for key in ("Param0", "Param1"):
                b[key] = b[key] * factor(size, b.get("Name"))
        for pd in doc["PDControllers"]:
            for key, spec in (("Kp", kp), ("Kd", kd), ("TorqueLim", torque_lim)):
                pd[key] = pd[key] * factor(spec, pd.get("Name"))
        text = json.dumps(doc)
        self.LoadVariantJson(v, text)
        return text

    def AssignVariants(self, env_ids, variants):
        """env_ids[i] -> variants[i] (env_ids None: the first len(variants) envs); takes effect with the env's next launch and leaves the env's state alone -- call
        Reset on those envs if their episodes are to START under the new model. Between frames only."""
        self._assign_keys(self._lib.dtrl_assign_variants, "AssignVariants", "variants", env_ids, variants)

    def GetVariants(self, env_ids=None):
        return self._get_keys(self._lib.dtrl_get_variants, env_ids)

    def VariantStats(self, v):
        """EvalStats restricted to the envs currently in variant v (plus their number), reduced on the device in a fixed order."""
        return self._key_stats(self._lib.dtrl_variant_stats, v)

    # ---- variant redraw: envs draw a new model variant at each episode start (no counterpart in the reference, which keeps one character per scene object) ----
    def VariantRedraw(self, lo, hi, seed=0, weights=None):
        """dtrl_variant_redraw: from now on an env whose variant is in lo .. hi (filled variants) draws a new variant of that range at every episode start -- the
        frame boundary at which it fell, or Reset naming it -- in front of the reset, which therefore runs under the new model. weights: None = uniform, else
        hi - lo + 1 non-negative numbers, not all zero. The draw depends on (seed, global env id, the env's own draw counter) alone. Envs outside lo .. hi are left
        alone. With -terrain_gen= device this happens on the device, without the host. VariantRedraw(1, 0) removes the redraw (variants and counters stay). With a
        redraw on device terrain, GetVariants / VariantRedrawInfo report the state as of the last completed frame boundary (not between UpdateBegin and UpdateEnd)."""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if int(lo) <= int(hi) and w.size != int(hi) - int(lo) + 1:
                raise DtrlError("VariantRedraw: weights must hold hi - lo + 1 = %d numbers, not %d" % (int(hi) - int(lo) + 1, w.size))
        self._chk(self._lib.dtrl_variant_redraw(self._h, int(lo), int(hi), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(w) if w is not None else None))

    def VariantRedrawInfo(self, env_ids=None):
        """dtrl_variant_redraw_info: {"lo", "hi" (the redraw's range), "variant", "draws" (int32 per listed env, all by default)}."""
        ids, n = self._ids(env_ids)
        lo, hi = C.c_int32(), C.c_int32()
        variant, draws = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self._lib.dtrl_variant_redraw_info(self._h, _p(ids), n, C.byref(lo), C.byref(hi), _p(variant), _p(draws)))
        return {"lo": int(lo.value), "hi": int(hi.value), "variant": variant, "draws": draws}

    # ---- variant rescale: per-episode continuous mass and motor scales, drawn on the device (no counterpart in the reference) ----
    def VariantRescale(self, base=0, env_ids=None, seed=0, mass=None, kp=None, kd=None, torque_lim=None, per_link=()):
        """dtrl_variant_rescale: from now on the listed envs (all by default; [] = the settings only) run under a private model record -- key num_variants + env
        id, at first a copy of variant `base` -- whose mass and motor scalars are redrawn at each of the env's episode starts: one factor per quantity from its
        range (lo, hi) (None = (1, 1): not scaled), for every link alike or, for the quantities named in per_link ("mass", "kp", "kd", "torque_lim"), one per
        link. The record then holds the bits ScaledVariant under the same factors would load. The draw depends on (seed, global env id, the env's episode
        number) alone. One small launch per env group and frame, no host wait. Costs sizeof(DevModel) more device memory per env. AssignVariants of an ordinary
        variant takes an env out; VariantRescale(None) removes the rescale (its envs go back to `base`, the counters stay)."""
        if base is None:
            self._chk(self._lib.dtrl_variant_rescale(self._h, 0, None, 0, 0, None))
            return
        unknown = set(per_link) - set(RESCALE_QUANTITIES)
        if unknown:
            raise DtrlError("VariantRescale: per_link names no quantity of the rescale: %s" % ", ".join(sorted(map(str, unknown))))
        d = RescaleDesc()
        for q, (name, r) in enumerate(zip(RESCALE_QUANTITIES, (mass, kp, kd, torque_lim))):
            lo, hi = (1.0, 1.0) if r is None else r
            getattr(d, name)[0], getattr(d, name)[1] = float(lo), float(hi)
            if name in per_link:
                d.per_link |= 1 << q
        ids, n = self._ids(env_ids)
        self._chk(self._lib.dtrl_variant_rescale(self._h, int(base), _p(ids), n, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(d)))

    def VariantRescaleInfo(self, env_ids=None):
        """dtrl_variant_rescale_info: {"base", "seed", "ranges" {quantity: (lo, hi)}, "per_link" (tuple of names), "key", "episodes" (int32 per listed env, all by
        default), "factors" [n, 4, L]: the factors of each env's CURRENT episode in RESCALE_QUANTITIES order, recomputed on the host by the library's rule from
        episodes - 1 (all 1 outside the rescale or before the first episode start)}."""
        ids, n = self._ids(env_ids)
        base, seed, d = C.c_int32(), C.c_uint64(), RescaleDesc()
        key, episodes = np.zeros(n, np.int32), np.zeros(n, np.int32)
        factors = np.zeros((n, 4, self.L), np.float64)
        self._chk(self._lib.dtrl_variant_rescale_info(self._h, _p(ids), n, C.byref(base), C.byref(seed), C.byref(d), _p(key), _p(episodes), _p(factors)))
        return {"base": int(base.value), "seed": int(seed.value), "ranges": {q: (getattr(d, q)[0], getattr(d, q)[1]) for q in RESCALE_QUANTITIES},
                "per_link": tuple(q for k, q in enumerate(RESCALE_QUANTITIES) if d.per_link >> k & 1), "key": key, "episodes": episodes, "factors": factors}

    def VariantScalars(self, env):
        """dtrl_variant_scalars: the mass and motor scalars of the model record env `env` runs under, read from the device table: ({"mass", "inertia", "sub_mass",
        "kp", "kd", "torque_lim"}: float64 [L], exact casts of the record's values; total_mass)."""
        out = np.zeros((6, self.L), np.float64); tm = C.c_double()
        self._chk(self._lib.dtrl_variant_scalars(self._h, int(env), _p(out), C.byref(tm)))
        return {k: out[r].copy() for r, k in enumerate(RESCALE_SCALARS)}, float(tm.value)

    # ---- terrain sets: several terrains in one batch, one per env (no counterpart in the reference, which keeps one terrain per scene object) ----
    num_terrains = 0

    def CreateTerrains(self, n_terrains):
        """dtrl_terrains_create: a table of 1 .. num_envs terrains (type + 40 parameters), once per batch. Terrain 0 is the batch's own terrain (SetTerrainLerp keeps
        acting on it) and every env starts in it; terrains >= 1 are empty until SetTerrainFile / SetTerrainParams fills them. Combines with policy slots, model
        variants and external policy mode."""
        self._chk(self._lib.dtrl_terrains_create(self._h, int(n_terrains)))
        self.num_terrains = int(n_terrains)

    def SetTerrainFile(self, t, path, lerp=0.0):
        """dtrl_terrain_set_file: terrain t >= 1 from a terrain file (resolved like -terrain_file=) at `lerp` over that file's parameter sets. Calling it again for a
        filled terrain moves that terrain's curriculum: its envs build their next segments under the new parameters."""
        self._chk(self._lib.dtrl_terrain_set_file(self._h, int(t), os.fsencode(str(path)), float(lerp)))

    def SetTerrainParams(self, t, type_name, params40):
        """dtrl_terrain_set_params: the same from memory (a type name and 40 parameters in cTerrainGen2D::eParams order, what terrain_build takes)."""
        p = np.ascontiguousarray(params40, np.float64)
        if p.shape != (40,):
            raise DtrlError("SetTerrainParams: params40 must hold 40 values")
        self._chk(self._lib.dtrl_terrain_set_params(self._h, int(t), str(type_name).encode(), _p(p)))

    def TerrainInfo(self, t):
        """dtrl_terrain_info: {"type", "params" (40 doubles), "filled"} of terrain t; terrain 0 reports the lerped parameters in force."""
        name = C.create_string_buffer(64); p = np.zeros(40, np.float64); filled = C.c_int()
        self._chk(self._lib.dtrl_terrain_info(self._h, int(t), name, 64, _p(p), C.byref(filled)))
        return {"type": name.value.decode(), "params": p, "filled": bool(filled.value)}

    def AssignTerrains(self, env_ids, terrains, restart=False):
        """env_ids[i] -> terrains[i] (env_ids None: the first len(terrains) envs). restart=False: takes effect with the env's next segment build, the window in place
        stays. restart=True: the listed envs start over as at creation under their new terrain (terrain stream re-seeded, fresh window, reset), in the same call."""
        self._assign_keys(self._lib.dtrl_assign_terrains, "AssignTerrains", "terrains", env_ids, terrains, 1 if restart else 0)

    def GetTerrains(self, env_ids=None):
        return self._get_keys(self._lib.dtrl_get_terrains, env_ids)

    def TerrainStats(self, t):
        """EvalStats restricted to the envs currently in terrain t (plus their number), reduced on the device in a fixed order."""
        return self._key_stats(self._lib.dtrl_terrain_stats, t)

    # ---- terrain ladder: envs climb and descend terrains lo .. hi by their own episodes (no counterpart in the reference, which keeps one terrain per scene object) ----
    def TerrainLadder(self, lo, hi, up_dist, down_dist, at_top=False):
        """dtrl_terrain_ladder: terrains lo .. hi (filled, ordered easy to hard) become a ladder. At each frame boundary an env that has come up_dist past its mark
        goes one level up (at the top: stays, or with at_top=True is dealt a level of the ladder at random), an env that falls within down_dist of its mark goes one
        down; envs in terrains outside lo .. hi are left alone. With -terrain_gen= device this happens inside the boundary launch, without the host. lo > hi removes
        the ladder. With a ladder, GetTerrains / LadderInfo report the state as of the last completed frame boundary (not between UpdateBegin and UpdateEnd)."""
        self._chk(self._lib.dtrl_terrain_ladder(self._h, int(lo), int(hi), float(up_dist), float(down_dist), 1 if at_top else 0))

    def LadderInfo(self, env_ids=None):
        """dtrl_ladder_info: {"mark_x" (float64: root x at the env's last spawn or level change), "ups", "downs" (int32)} of the listed envs (all by default)."""
        ids, n = self._ids(env_ids)
        mark, ups, downs = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self._lib.dtrl_ladder_info(self._h, _p(ids), n, _p(mark), _p(ups), _p(downs)))
        return {"mark_x": mark, "ups": ups, "downs": downs}

    # ---- full env snapshots (no counterpart in the reference: it keeps one scene per object) ----
    def SaveState(self, env_ids=None):
        """Save everything that decides the listed envs' future (all envs by default) into a device-resident Snapshot. Not between UpdateBegin and UpdateEnd."""
        ids, n = self._ids(env_ids)
        h = C.c_void_p()
        self._chk(self._lib.dtrl_snapshot_save(self._h, _p(ids), n, C.byref(h)))
        return Snapshot(self, h)

    def RestoreState(self, snap, env_ids=None):
        """Put the saved envs back into their own slots, or -- env_ids given -- the first len(env_ids) saved envs into those slots (transplant: the env then
        continues with the exploration stream of its new slot)."""
        ids, n = self._ids(env_ids)
        self._chk(self._lib.dtrl_snapshot_restore(self._h, snap._h, _p(ids), n if ids is not None else 0))

    def CloneEnvs(self, src, dst):
        """Env dst[i] becomes a copy of env src[i]; overlapping lists behave as read-all-then-write-all."""
        s = np.ascontiguousarray(src, np.int32); d = np.ascontiguousarray(dst, np.int32)
        if s.shape != d.shape or s.ndim != 1:
            raise DtrlError("CloneEnvs: src and dst must be lists of the same length")
        self._chk(self._lib.dtrl_clone_envs(self._h, _p(s), _p(d), len(s)))

    def ImportState(self, blob):
        """A blob written by Snapshot.export() (this or another process, same character / precision / terrain mode) -> a Snapshot held by this batch."""
        raw = np.frombuffer(bytes(blob), np.uint8)
        h = C.c_void_p()
        self._chk(self._lib.dtrl_snapshot_import(self._h, _p(raw), raw.size, C.byref(h)))
        return Snapshot(self, h)

    def KernelTimeMs(self):
        a = C.c_double(); n = C.c_int64()
        self._chk(self._lib.dtrl_kernel_time_ms(self._h, C.byref(a), C.byref(n)))
        return a.value, n.value


def version():
    return _bind(LIB_PATH).dtrl_version().decode()


# ---- host-side utility entry points (no batch, no device) ----
def terrain_build(type_name, params40, seed, width):
    """cTerrainGen2D::GetTerrainFunc(type)(width, params, cRand(seed), data): (float32 heights, width added)."""
    L = _bind(LIB_PATH)
    p = np.ascontiguousarray(params40, np.float64); buf = np.zeros(8192, np.float32); n = C.c_int(); w = C.c_double()
    rc = L.dtrl_terrain_build(type_name.encode(), _p(p), int(seed), float(width), _p(buf), 8192, C.byref(n), C.byref(w))
    if rc != DTRL_OK:
        raise DtrlError("dtrl_terrain_build failed (%d): %s" % (rc, L.dtrl_last_error(None).decode()))
    return buf[:n.value].copy(), w.value


def terrain_load_file(path, max_sets=8):
    """Terrain file -> (type name, [n_sets, 40] parameter vectors in cTerrainGen2D::eParams order)."""
    L = _bind(LIB_PATH)
    buf = C.create_string_buffer(64); prm = np.zeros((max_sets, 40)); n = C.c_int()
    rc = L.dtrl_terrain_load_file(os.fsencode(path), buf, 64, _p(prm), max_sets, C.byref(n))
    if rc != DTRL_OK:
        raise DtrlError("dtrl_terrain_load_file failed (%d): %s" % (rc, L.dtrl_last_error(None).decode()))
    return buf.value.decode(), prm[:n.value].copy()


def args_parse_string(argv, key):
    """cArgParser(argv) + AppendArgs(-arg_file=) + ParseString(key): (value or None, number of tokens)."""
    L = _bind(LIB_PATH)
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    buf = C.create_string_buffer(4096); found = C.c_int(); nt = C.c_int()
    rc = L.dtrl_args_parse_string(arr, len(argv), key.encode(), buf, 4096, C.byref(found), C.byref(nt))
    if rc != DTRL_OK:
        raise DtrlError("dtrl_args_parse_string failed (%d): %s" % (rc, L.dtrl_last_error(None).decode()))
    return (buf.value.decode() if found.value else None), nt.value
