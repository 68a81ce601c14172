"""ppamd — Python bindings (ctypes) over the C-ABI in include/pp.h.

The compute path is the HIP library ``libppamd.so`` built for gfx950 from ``csrc/``; this module
only marshals buffers. Importing it fails loudly if the library is missing: there is no CPU
fallback for the planner (the CPU restatement under ``oracle/`` is test infrastructure only).

Reference interface mirrored: the per-frame ``onMessage`` compute body of
Fable3/CarND-Path-Planning-Project ``src/main.cpp:1229-1457`` (see ``plan_frame``) and, batched,
``TrajectoryBuilder::build`` over a (lane, target speed) candidate grid (see ``evaluate``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPAMD_LIB") or os.path.join(_HERE, "libppamd.so")   # override: A/B builds


def lib_sha256(path=None):
    """SHA-256 of the loaded HIP library file (bench.py matches profile summaries against it)."""
    import hashlib
    h = hashlib.sha256()
    with open(path or LIB_PATH, "rb") as f:
        for b in iter(lambda: f.read(1 << 20), b""):
            h.update(b)
    return h.hexdigest()

def _open():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"ppamd: HIP library not built: {LIB_PATH} (run __graft_entry__.build())")
    # torch (ROCm) bundles its own libamdhip64 (soname libamdhip64.so.7, loaded by path). Load it
    # first so that our DT_NEEDED libamdhip64.so.7 resolves to that same runtime: two HIP runtimes
    # in one process do not share device allocations.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    h = C.CDLL(LIB_PATH)
    h.pp_num_lanes.restype = C.c_int32
    return h


_LIB = _open()
NUM_LANES = int(_LIB.pp_num_lanes())   # PP_NUM_LANES the library was built for (src/main.cpp:22)
PREV_KEEP = 10
_LIB.pp_max_cars.restype = C.c_int32
MAX_CARS = int(_LIB.pp_max_cars())     # PP_MAX_CARS: sensor_fusion rows and car-table slots per scene
MAX_SPEEDS = 8
MAX_POINTS = 128

COST_REFERENCE = 0
COST_COMFORT = 1

STATUS_BITS = {
    "EGO_UNMATCHED": 1 << 0, "CAR_UNMATCHED": 1 << 1, "FALLBACK": 1 << 2, "SPLINE_TRUNC": 1 << 3,
    "NAN": 1 << 4, "COLLISION": 1 << 5, "ACC_OVERRIDE": 1 << 6, "CURV_ADJUST": 1 << 7,
    "TOO_FAR": 1 << 8, "BRAKE": 1 << 9, "MAXBRAKE": 1 << 10, "ADJUST": 1 << 11, "KEEP": 1 << 12,
    "LANE_CLOSED": 1 << 13, "JUMP_RULE": 1 << 14,
}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)


class SceneBatch(C.Structure):
    _fields_ = [("n_scenes", C.c_int64), ("car_stride", C.c_int32), ("tab_slots", C.c_int32),
                ("ego_x", C.c_void_p), ("ego_y", C.c_void_p), ("ego_yaw_deg", C.c_void_p),
                ("ego_speed_mph", C.c_void_p), ("prev_x", C.c_void_p), ("prev_y", C.c_void_p),
                ("n_prev", C.c_void_p), ("prev_target_lane", C.c_void_p), ("n_cars", C.c_void_p),
                ("car_id", C.c_void_p), ("car_x", C.c_void_p), ("car_y", C.c_void_p),
                ("car_vx", C.c_void_p), ("car_vy", C.c_void_p),
                ("tab_id", C.c_void_p), ("tab_valid", C.c_void_p), ("tab_lane", C.c_void_p), ("tab_s", C.c_void_p),
                ("tab_d", C.c_void_p), ("tab_vs", C.c_void_p), ("tab_vd", C.c_void_p),
                ("tab_vx", C.c_void_p), ("tab_vy", C.c_void_p)]

TABLE_FIELDS_I = ["tab_id", "tab_valid", "tab_lane"]
TABLE_FIELDS_F = ["tab_s", "tab_d", "tab_vs", "tab_vd", "tab_vx", "tab_vy"]


class Traffic(C.Structure):
    _fields_ = [("n_cars", C.c_int32), ("_pad", C.c_int32), ("lane", C.c_void_p), ("seg", C.c_void_p),
                ("t", C.c_void_p), ("offset", C.c_void_p), ("speed", C.c_void_p)]


class ServerOpts(C.Structure):
    _fields_ = [("host", C.c_char_p), ("port", C.c_int32), ("max_clients", C.c_int32), ("n_speeds", C.c_int32),
                ("threads", C.c_int32), ("device", C.c_int32), ("_pad", C.c_int32), ("max_frames", C.c_int64)]


class RolloutCfg(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("consume", C.c_int32), ("sensor_range", C.c_double)]


LOG_FIELDS = [("ego_x", "f8"), ("ego_y", "f8"), ("ego_speed_mph", "f8"), ("target_lane", "i4"),
              ("winner", "i4"), ("n_out", "i4"), ("status", "u4"), ("n_cars", "i4")]


class RolloutLog(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in LOG_FIELDS] + [("plan_x", C.c_void_p), ("plan_y", C.c_void_p)]


class JudgeCfg(C.Structure):
    _fields_ = [("speed_limit_mph", C.c_double), ("max_acc", C.c_double), ("max_jerk", C.c_double),
                ("ego_length", C.c_double), ("ego_width", C.c_double), ("car_length", C.c_double),
                ("car_width", C.c_double), ("lane_tol", C.c_double), ("acc_window", C.c_int32),
                ("jerk_window", C.c_int32), ("off_lane_steps", C.c_int32), ("_pad", C.c_int32)]


# The states' field tables: name, dtype, leading dimension (None: [S], a number k: [k, S], "n": [n, S],
# one row per car). The rollout judge's state (include/pp.h pp_judge):
JUDGE_RING = 64
INC_KINDS = ["COLLISION", "SPEED", "ACC", "JERK", "OFF_LANE"]      # kind k is flag bit 1 << k
INC_COLLISION, INC_SPEED, INC_ACC, INC_JERK, INC_OFF_LANE = (1 << k for k in range(5))
JUDGE_FIELDS = [("steps", "i4", None), ("flags", "u4", None), ("count", "i4", len(INC_KINDS)),
                ("first_step", "i4", len(INC_KINDS)), ("first_car", "i4", None), ("seg_hint", "i4", None),
                ("off_run", "i4", None), ("head_x", "f8", None), ("head_y", "f8", None),
                ("ring_vx", "f8", JUDGE_RING), ("ring_vy", "f8", JUDGE_RING), ("dist", "f8", None),
                ("clean_dist", "f8", None), ("min_sep", "f8", None), ("max_speed_mph", "f8", None),
                ("max_acc", "f8", None), ("max_jerk", "f8", None)]


class Judge(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in JUDGE_FIELDS]


class FollowCfg(C.Structure):
    _fields_ = [("max_acc", C.c_double), ("comfort_brake", C.c_double), ("max_brake", C.c_double),
                ("time_headway", C.c_double), ("min_gap", C.c_double), ("gap_floor", C.c_double),
                ("horizon", C.c_double), ("car_length", C.c_double), ("ego_length", C.c_double),
                ("lateral_reach", C.c_double), ("react_to_ego", C.c_int32), ("_pad", C.c_int32)]


# reactive traffic's state (include/pp.h pp_follow)
FOLLOW_FIELDS = [("started", "i4", None), ("ego_seg", "i4", None), ("desired", "f8", "n"),
                 ("next_speed", "f8", "n"), ("leader", "i4", "n"), ("gap", "f8", "n")]


class Follow(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in FOLLOW_FIELDS]


class LaneChangeCfg(C.Structure):
    _fields_ = [("politeness", C.c_double), ("threshold", C.c_double), ("right_bias", C.c_double),
                ("safe_brake", C.c_double), ("lateral_speed", C.c_double), ("ego_desired_speed", C.c_double),
                ("min_interval_steps", C.c_int32), ("_pad", C.c_int32)]


# lane-changing traffic's state (include/pp.h pp_lane_change)
LANE_CHANGE_FIELDS = [("started", "i4", None), ("n_changes", "i4", None), ("last_car", "i4", None),
                      ("last_dir", "i4", None), ("home", "f8", "n"), ("wait", "i4", "n"), ("changes", "i4", "n"),
                      ("arc", "f8", "n"), ("gain", "f8", "n"), ("dir", "i4", "n")]


class LaneChange(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in LANE_CHANGE_FIELDS]


class SensorCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_scene", C.c_int64), ("pos_sigma", C.c_double),
                ("pos_sigma_per_m", C.c_double), ("vel_sigma", C.c_double), ("dropout_prob", C.c_double),
                ("occlusion_radius", C.c_double)]


# the sensor model's state (include/pp.h pp_sensor); "r": [car_stride, S], one row per telemetry row
SENSE_NONE, SENSE_REPORTED, SENSE_OCCLUDED, SENSE_DROPPED = range(4)
SENSOR_FIELDS = [("frame", "i4", None), ("n_cars", "i4", None), ("car_id", "i4", "n"), ("car_x", "f8", "n"),
                 ("car_y", "f8", "n"), ("car_vx", "f8", "n"), ("car_vy", "f8", "n"), ("fate", "i4", "n")]
SENSED_ROWS = ["n_cars", "car_id", "car_x", "car_y", "car_vx", "car_vy"]      # what replaces the truth's for pp_eval


class Sensor(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in SENSOR_FIELDS]


class TrackerCfg(C.Structure):
    _fields_ = [("meas_pos_sigma", C.c_double), ("meas_pos_sigma_per_m", C.c_double), ("meas_vel_sigma", C.c_double),
                ("acc_sigma", C.c_double), ("max_coast", C.c_int32), ("_pad", C.c_int32)]


# the tracker's state (include/pp.h pp_tracker); "2n": [2 car_stride, S], the two banks of track slots
TRACK_NONE, TRACK_NEW, TRACK_UPDATED, TRACK_COASTED = range(4)
TRACK_SLOT_FIELDS = ["id", "misses", "x", "y", "vx", "vy", "ppp", "ppv", "pvv"]
TRACKER_FIELDS = ([("frame", "i4", None), ("n_tracks", "i4", 2), ("id", "i4", "2n"), ("misses", "i4", "2n")] +
                  [(k, "f8", "2n") for k in TRACK_SLOT_FIELDS[2:]] +
                  [("n_cars", "i4", None), ("car_id", "i4", "n"), ("car_x", "f8", "n"), ("car_y", "f8", "n"),
                   ("car_vx", "f8", "n"), ("car_vy", "f8", "n"), ("src", "i4", "n")])


class Tracker(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in TRACKER_FIELDS]


class EpisodeCfg(C.Structure):
    _fields_ = [("n_cars", C.c_int32), ("_pad", C.c_int32), ("ego_speed_min", C.c_double),
                ("ego_speed_max", C.c_double), ("car_speed_min", C.c_double), ("car_speed_max", C.c_double),
                ("ahead_share", C.c_double), ("extra_gap", C.c_double), ("offset_jitter", C.c_double),
                ("gap_slack", C.c_double)]


class SummaryCfg(C.Structure):
    _fields_ = [("scenes_per_group", C.c_int64), ("hist_bins", C.c_int32), ("_pad", C.c_int32),
                ("hist_max", C.c_double), ("out_first", C.c_int64), ("out_stride", C.c_int64)]


# the judge summary's rows (include/pp.h pp_judge_stats): name, dtype, leading dimension (None: [R],
# a number k: [k, R], "b": [hist_bins, R])
STATS_MAX_BINS = 1024
STATS_FIELDS = [("n_scenes", "i8", None), ("n_unjudged", "i8", None), ("n_nonfinite", "i8", None),
                ("n_clean", "i8", None), ("steps", "i8", None), ("scenes_with", "i8", len(INC_KINDS)),
                ("steps_in", "i8", len(INC_KINDS)), ("first_step_min", "i4", len(INC_KINDS)),
                ("dist_sum", "f8", None), ("clean_dist_sum", "f8", None), ("clean_dist_min", "f8", None),
                ("clean_dist_max", "f8", None), ("min_sep", "f8", None), ("max_speed_mph", "f8", None),
                ("max_acc", "f8", None), ("max_jerk", "f8", None), ("hist", "i8", "b")]


class JudgeStats(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in STATS_FIELDS]


class Params(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_speeds", C.c_int32), ("cost_mode", C.c_int32),
                ("emit_paths", C.c_int32), ("speed_offsets", C.c_double * MAX_SPEEDS),
                ("relaxed_acc", C.c_double), ("min_relaxed_acc_while_braking", C.c_double),
                ("maximum_acc", C.c_double), ("max_speed", C.c_double), ("car_length", C.c_double),
                ("safety_distance", C.c_double), ("keep_distance", C.c_double),
                ("keep_distance_leeway", C.c_double), ("n_draws", C.c_int32), ("_pad_mc", C.c_int32),
                ("noise_seed", C.c_uint64), ("noise_first_scene", C.c_int64),
                ("noise_pos_sigma", C.c_double), ("noise_vel_sigma", C.c_double)]


class SweepCfg(C.Structure):
    _fields_ = [("n_sets", C.c_int32), ("_pad", C.c_int32), ("seed", C.c_uint64), ("first_scene", C.c_int64),
                ("rollout", RolloutCfg), ("summary", SummaryCfg)]


class SceneInfo(C.Structure):
    _fields_ = [("ego_x", C.c_double), ("ego_y", C.c_double), ("ego_speed", C.c_double),
                ("ego_acc", C.c_double), ("ego_s", C.c_double), ("ego_d", C.c_double),
                ("ego_vs", C.c_double), ("ego_vd", C.c_double), ("ref_ratio", C.c_double * NUM_LANES),
                ("lane_score", C.c_double * NUM_LANES), ("ref_wp", C.c_int32), ("ego_lane", C.c_int32),
                ("target_lane", C.c_int32), ("lane_open_mask", C.c_int32),
                ("n_matched_cars", C.c_int32), ("in_lane_car", C.c_int32), ("_pad", C.c_int32 * 2)]


INFO_DTYPE = np.dtype([("ego_x", "f8"), ("ego_y", "f8"), ("ego_speed", "f8"), ("ego_acc", "f8"),
                       ("ego_s", "f8"), ("ego_d", "f8"), ("ego_vs", "f8"), ("ego_vd", "f8"),
                       ("ref_ratio", "f8", NUM_LANES), ("lane_score", "f8", NUM_LANES), ("ref_wp", "i4"),
                       ("ego_lane", "i4"), ("target_lane", "i4"), ("lane_open_mask", "i4"),
                       ("n_matched_cars", "i4"), ("in_lane_car", "i4"), ("_pad", "i4", 2)])
assert INFO_DTYPE.itemsize == C.sizeof(SceneInfo)


class Result(C.Structure):
    _fields_ = [("winner", C.c_void_p), ("n_out", C.c_void_p), ("next_x", C.c_void_p),
                ("next_y", C.c_void_p), ("cost", C.c_void_p), ("status", C.c_void_p),
                ("paths", C.c_void_p), ("path_len", C.c_void_p), ("info", C.c_void_p),
                ("draw_mean_cost", C.c_void_p)]


# exported symbols of include/pp.h (checked by tests/test_capi.py; pp_sensor_word, the one function that
# returns a uint32_t, is bound below as well)
EXPORTS = ["pp_params_default", "pp_num_candidates", "pp_version", "pp_map_create",
           "pp_map_destroy", "pp_map_geometry", "pp_reserve", "pp_eval", "pp_plan_frame",
           "pp_synth_scenes", "pp_synth_scenes_host", "pp_timing_enable", "pp_timing_read",
           "pp_mc_gauss", "pp_rollout", "pp_synth_traffic", "pp_synth_traffic_host", "pp_plan_reset",
           "pp_telemetry_parse", "pp_control_format", "pp_plan_batch_host", "pp_serve", "pp_ws_accept_key",
           "pp_telemetry_parse_device", "pp_control_format_device", "pp_map_create_device",
           "pp_num_lanes", "pp_max_cars", "pp_libm_eval", "pp_debug_set", "pp_debug_get",
           "pp_judge_cfg_default", "pp_judge_frame", "pp_judge_frame_host", "pp_rollout_judged",
           "pp_follow_cfg_default", "pp_traffic_follow", "pp_traffic_follow_host", "pp_rollout_reactive",
           "pp_episode_cfg_default", "pp_synth_episode", "pp_synth_episode_host", "pp_math_eval",
           "pp_lane_change_cfg_default", "pp_traffic_lane_change", "pp_traffic_lane_change_host",
           "pp_rollout_lane_changing", "pp_judge_summary", "pp_judge_summary_host", "pp_rollout_sweep",
           "pp_sensor_cfg_default", "pp_sense_frame", "pp_sense_frame_host", "pp_sensor_gauss", "pp_rollout_sensed",
           "pp_rollout_sweep_sensed", "pp_tracker_cfg_default", "pp_track_frame", "pp_track_frame_host",
           "pp_rollout_tracked", "pp_rollout_sweep_tracked"]


def _load():
    lib = _LIB
    lib.pp_params_default.argtypes = [C.POINTER(Params)]
    lib.pp_params_default.restype = None
    lib.pp_num_candidates.argtypes = [C.POINTER(Params)]
    lib.pp_num_candidates.restype = C.c_int32
    lib.pp_version.restype = C.c_char_p
    lib.pp_map_create.argtypes = [_dp, _dp, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pp_map_create.restype = C.c_int32
    lib.pp_map_create_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.POINTER(C.c_void_p)]
    lib.pp_map_create_device.restype = C.c_int32
    lib.pp_map_destroy.argtypes = [C.c_void_p]
    lib.pp_map_destroy.restype = C.c_int32
    lib.pp_map_geometry.argtypes = [C.c_void_p, _dp, C.c_int32]
    lib.pp_map_geometry.restype = C.c_int32
    lib.pp_reserve.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
    lib.pp_reserve.restype = C.c_int32
    lib.pp_eval.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Params),
                            C.POINTER(Result), C.c_int32, C.c_void_p]
    lib.pp_eval.restype = C.c_int32
    lib.pp_synth_scenes.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(SceneBatch),
                                    C.c_int32, C.c_void_p]
    lib.pp_synth_scenes.restype = C.c_int32
    lib.pp_synth_scenes_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(SceneBatch)]
    lib.pp_synth_scenes_host.restype = C.c_int32
    lib.pp_plan_frame.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double,
                                  C.c_double, _dp, _dp, C.c_int32, _ip, _dp, _dp, _dp, _dp,
                                  C.c_int32, _ip, _dp, _dp, _ip]
    lib.pp_plan_frame.restype = C.c_int32
    lib.pp_debug_set.argtypes = [C.c_int32, C.c_int32]
    lib.pp_debug_set.restype = C.c_int32
    lib.pp_debug_get.argtypes = [C.c_int32]
    lib.pp_debug_get.restype = C.c_int32
    lib.pp_timing_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.pp_timing_enable.restype = C.c_int32
    lib.pp_timing_read.argtypes = [C.c_void_p, C.c_int32, _dp, C.POINTER(C.c_int64)]
    lib.pp_timing_read.restype = C.c_int32
    lib.pp_mc_gauss.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.pp_mc_gauss.restype = C.c_double
    lib.pp_rollout.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Params),
                               C.POINTER(RolloutCfg), C.POINTER(Result), C.POINTER(RolloutLog), C.c_int32,
                               C.c_void_p]
    lib.pp_rollout.restype = C.c_int32
    lib.pp_judge_cfg_default.argtypes = [C.POINTER(JudgeCfg)]
    lib.pp_judge_cfg_default.restype = None
    lib.pp_judge_frame.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Result),
                                   C.c_int32, C.POINTER(JudgeCfg), C.POINTER(Judge), C.c_int32, C.c_void_p]
    lib.pp_judge_frame.restype = C.c_int32
    lib.pp_judge_frame_host.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Result),
                                        C.c_int32, C.POINTER(JudgeCfg), C.POINTER(Judge)]
    lib.pp_judge_frame_host.restype = C.c_int32
    lib.pp_rollout_judged.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Params),
                                      C.POINTER(RolloutCfg), C.POINTER(Result), C.POINTER(RolloutLog), C.c_int32,
                                      C.c_void_p, C.POINTER(JudgeCfg), C.POINTER(Judge)]
    lib.pp_rollout_judged.restype = C.c_int32
    lib.pp_follow_cfg_default.argtypes = [C.POINTER(FollowCfg)]
    lib.pp_follow_cfg_default.restype = None
    lib.pp_traffic_follow.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.c_int32,
                                      C.POINTER(FollowCfg), C.POINTER(Follow), C.c_int32, C.c_void_p]
    lib.pp_traffic_follow.restype = C.c_int32
    lib.pp_traffic_follow_host.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.c_int32,
                                           C.POINTER(FollowCfg), C.POINTER(Follow)]
    lib.pp_traffic_follow_host.restype = C.c_int32
    lib.pp_rollout_reactive.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Params),
                                        C.POINTER(RolloutCfg), C.POINTER(Result), C.POINTER(RolloutLog), C.c_int32,
                                        C.c_void_p, C.POINTER(JudgeCfg), C.POINTER(Judge), C.POINTER(FollowCfg),
                                        C.POINTER(Follow)]
    lib.pp_rollout_reactive.restype = C.c_int32
    lib.pp_lane_change_cfg_default.argtypes = [C.POINTER(LaneChangeCfg)]
    lib.pp_lane_change_cfg_default.restype = None
    lib.pp_traffic_lane_change.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.c_int32,
                                           C.POINTER(FollowCfg), C.POINTER(Follow), C.POINTER(LaneChangeCfg),
                                           C.POINTER(LaneChange), C.c_int32, C.c_void_p]
    lib.pp_traffic_lane_change.restype = C.c_int32
    lib.pp_traffic_lane_change_host.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic), C.c_int32,
                                                C.POINTER(FollowCfg), C.POINTER(Follow), C.POINTER(LaneChangeCfg),
                                                C.POINTER(LaneChange)]
    lib.pp_traffic_lane_change_host.restype = C.c_int32
    lib.pp_rollout_lane_changing.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(Traffic),
                                             C.POINTER(Params), C.POINTER(RolloutCfg), C.POINTER(Result),
                                             C.POINTER(RolloutLog), C.c_int32, C.c_void_p, C.POINTER(JudgeCfg),
                                             C.POINTER(Judge), C.POINTER(FollowCfg), C.POINTER(Follow),
                                             C.POINTER(LaneChangeCfg), C.POINTER(LaneChange)]
    lib.pp_rollout_lane_changing.restype = C.c_int32
    lib.pp_judge_summary.argtypes = [C.c_void_p, C.POINTER(Judge), C.c_int64, C.POINTER(SummaryCfg),
                                     C.POINTER(JudgeStats), C.c_int32, C.c_void_p]
    lib.pp_judge_summary.restype = C.c_int32
    lib.pp_judge_summary_host.argtypes = [C.POINTER(Judge), C.c_int64, C.POINTER(SummaryCfg), C.POINTER(JudgeStats)]
    lib.pp_judge_summary_host.restype = C.c_int32
    lib.pp_rollout_sweep.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(SweepCfg), C.POINTER(EpisodeCfg),
                                     C.POINTER(JudgeCfg), C.POINTER(FollowCfg), C.POINTER(LaneChangeCfg),
                                     C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Result), C.POINTER(Judge),
                                     C.POINTER(Follow), C.POINTER(LaneChange), C.POINTER(JudgeStats), C.c_int32,
                                     C.c_void_p]
    lib.pp_rollout_sweep.restype = C.c_int32
    lib.pp_sensor_cfg_default.argtypes = [C.POINTER(SensorCfg)]
    lib.pp_sensor_cfg_default.restype = None
    lib.pp_sense_frame.argtypes = [C.POINTER(SceneBatch), C.POINTER(SensorCfg), C.POINTER(Sensor), C.c_int32,
                                   C.c_void_p]
    lib.pp_sense_frame.restype = C.c_int32
    lib.pp_sense_frame_host.argtypes = [C.POINTER(SceneBatch), C.POINTER(SensorCfg), C.POINTER(Sensor)]
    lib.pp_sense_frame_host.restype = C.c_int32
    lib.pp_sensor_gauss.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.pp_sensor_gauss.restype = C.c_double
    lib.pp_sensor_word.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32]
    lib.pp_sensor_word.restype = C.c_uint32
    lib.pp_rollout_sensed.argtypes = lib.pp_rollout_lane_changing.argtypes + [C.POINTER(SensorCfg), C.POINTER(Sensor)]
    lib.pp_rollout_sensed.restype = C.c_int32
    lib.pp_rollout_sweep_sensed.argtypes = lib.pp_rollout_sweep.argtypes + [C.POINTER(SensorCfg), C.POINTER(Sensor)]
    lib.pp_rollout_sweep_sensed.restype = C.c_int32
    lib.pp_tracker_cfg_default.argtypes = [C.POINTER(TrackerCfg)]
    lib.pp_tracker_cfg_default.restype = None
    lib.pp_track_frame.argtypes = [C.POINTER(SceneBatch), C.POINTER(TrackerCfg), C.c_int32, C.POINTER(Tracker),
                                   C.c_int32, C.c_void_p]
    lib.pp_track_frame.restype = C.c_int32
    lib.pp_track_frame_host.argtypes = [C.POINTER(SceneBatch), C.POINTER(TrackerCfg), C.c_int32, C.POINTER(Tracker)]
    lib.pp_track_frame_host.restype = C.c_int32
    lib.pp_rollout_tracked.argtypes = lib.pp_rollout_sensed.argtypes + [C.POINTER(TrackerCfg), C.POINTER(Tracker)]
    lib.pp_rollout_tracked.restype = C.c_int32
    lib.pp_rollout_sweep_tracked.argtypes = lib.pp_rollout_sweep_sensed.argtypes + [C.POINTER(TrackerCfg),
                                                                                    C.POINTER(Tracker)]
    lib.pp_rollout_sweep_tracked.restype = C.c_int32
    lib.pp_synth_traffic.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(SceneBatch),
                                     C.POINTER(Traffic), C.c_int32, C.c_void_p]
    lib.pp_synth_traffic.restype = C.c_int32
    lib.pp_synth_traffic_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(SceneBatch),
                                          C.POINTER(Traffic)]
    lib.pp_synth_traffic_host.restype = C.c_int32
    lib.pp_episode_cfg_default.argtypes = [C.POINTER(EpisodeCfg)]
    lib.pp_episode_cfg_default.restype = None
    lib.pp_synth_episode.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(EpisodeCfg), C.POINTER(FollowCfg),
                                     C.POINTER(SceneBatch), C.POINTER(Traffic), C.POINTER(Judge), C.POINTER(Follow),
                                     C.c_int32, C.c_void_p]
    lib.pp_synth_episode.restype = C.c_int32
    lib.pp_synth_episode_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(EpisodeCfg),
                                          C.POINTER(FollowCfg), C.POINTER(SceneBatch), C.POINTER(Traffic),
                                          C.POINTER(Judge), C.POINTER(Follow)]
    lib.pp_synth_episode_host.restype = C.c_int32
    lib.pp_plan_reset.argtypes = [C.c_void_p, C.c_int32]
    lib.pp_plan_reset.restype = C.c_int32
    lib.pp_telemetry_parse.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(SceneBatch),
                                       C.POINTER(C.c_int32), C.c_int32]
    lib.pp_telemetry_parse.restype = C.c_int32
    lib.pp_control_format.argtypes = [_dp, _dp, C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_char_p,
                                      C.c_int64, C.POINTER(C.c_int64), C.c_int32]
    lib.pp_control_format.restype = C.c_int32
    lib.pp_plan_batch_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(SceneBatch), C.POINTER(Params),
                                       C.POINTER(Result), C.c_void_p]
    lib.pp_plan_batch_host.restype = C.c_int32
    lib.pp_serve.argtypes = [C.c_void_p, C.POINTER(ServerOpts), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                             C.POINTER(C.c_int64)]
    lib.pp_serve.restype = C.c_int32
    lib.pp_ws_accept_key.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
    lib.pp_ws_accept_key.restype = C.c_int32
    lib.pp_telemetry_parse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SceneBatch), C.c_void_p,
                                              C.c_int32, C.c_void_p]
    lib.pp_telemetry_parse_device.restype = C.c_int32
    lib.pp_control_format_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    lib.pp_control_format_device.restype = C.c_int32
    lib.pp_libm_eval.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.pp_libm_eval.restype = C.c_int32
    lib.pp_math_eval.argtypes = [C.c_int32] + [C.c_void_p] * 7 + [C.c_int64, C.c_int32, C.c_void_p]
    lib.pp_math_eval.restype = C.c_int32
    return lib


lib = _load()


class PPError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise PPError(f"{what} failed with status {rc}")


def default_params(n_speeds=5, n_points=50, cost_mode=COST_REFERENCE, emit_paths=False,
                   speed_offsets=None, n_draws=0, noise_seed=None, noise_first_scene=0) -> Params:
    p = Params()
    lib.pp_params_default(C.byref(p))
    p.n_speeds = n_speeds
    p.n_points = n_points
    p.cost_mode = cost_mode
    p.emit_paths = 1 if emit_paths else 0
    p.n_draws = n_draws
    if noise_seed is not None:
        p.noise_seed = noise_seed
    p.noise_first_scene = noise_first_scene
    if speed_offsets is not None:
        for i, v in enumerate(speed_offsets):
            p.speed_offsets[i] = float(v)
    return p


def _ptr(a):
    """Data pointer of a numpy array or torch tensor (contiguous)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    assert a.is_contiguous()
    return a.data_ptr()


def _ref(x):
    """byref of a ctypes structure; None (a null pointer) for None."""
    return C.byref(x) if x is not None else None


def _zeros(xp, device):
    """mk(shape, dtype code): a zero array, numpy on the host or torch on `device` (torch holds the
    u4 words as int32: it has no uint32 arithmetic; *_to_numpy view them back)."""
    if xp == "numpy":
        return lambda sh, dt: np.zeros(sh, dt)
    import torch
    tdt = {"f8": torch.float64, "i4": torch.int32, "u4": torch.int32, "i8": torch.int64}
    return lambda sh, dt: torch.zeros(sh, dtype=tdt[dt], device=device)


def _alloc_state(fields, S, n, xp, device):
    """Zero arrays of a field table (JUDGE_FIELDS, FOLLOW_FIELDS, LANE_CHANGE_FIELDS)."""
    mk = _zeros(xp, device)
    rows = lambda lead: n if lead == "n" else (2 * n if lead == "2n" else lead)
    return {k: mk((S,) if lead is None else (rows(lead), S), dt) for k, dt, lead in fields}


def _struct(cls, names, d, optional=False):
    """A pointer structure from the arrays of dict d; optional: a missing array is a null pointer."""
    s = cls()
    for k in names:
        setattr(s, k, _ptr(d.get(k) if optional else d[k]))
    return s


def _to_numpy(d):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in d.items()}


def _default_cfg(cls, fill, over):
    """A configuration structure filled by the library's pp_*_cfg_default, fields overridden by keyword."""
    c = cls()
    fill(C.byref(c))
    for k, v in over.items():
        if k not in dict(cls._fields_):
            raise KeyError(k)
        setattr(c, k, v)
    return c


class Map:
    """Map::Init (src/main.cpp:89-131) over waypoint x/y; lane geometry uploaded per device."""

    def __init__(self, wx, wy):
        self.wx = np.ascontiguousarray(wx, dtype=np.float64)
        self.wy = np.ascontiguousarray(wy, dtype=np.float64)
        self.n = len(self.wx)
        h = C.c_void_p()
        _check(lib.pp_map_create(self.wx.ctypes.data_as(_dp), self.wy.ctypes.data_as(_dp),
                                 self.n, C.byref(h)), "pp_map_create")
        self.handle = h

    @classmethod
    def from_device(cls, d_wx, d_wy, device=0, stream=None):
        """pp_map_create_device: Map::Init on the GPU from torch waypoint tensors."""
        self = cls.__new__(cls)
        self.wx = d_wx.detach().cpu().numpy().astype(np.float64)
        self.wy = d_wy.detach().cpu().numpy().astype(np.float64)
        self.n = len(self.wx)
        h = C.c_void_p()
        _check(lib.pp_map_create_device(d_wx.data_ptr(), d_wy.data_ptr(), self.n, device, stream, C.byref(h)),
               "pp_map_create_device")
        self.handle = h
        return self

    def geometry(self) -> np.ndarray:
        out = np.zeros((self.n, 4 + 2 * NUM_LANES), np.float64)
        _check(lib.pp_map_geometry(self.handle, out.ctypes.data_as(_dp), self.n), "pp_map_geometry")
        return out

    def reserve(self, device, max_scenes):
        _check(lib.pp_reserve(self.handle, device, max_scenes), "pp_reserve")

    def timing(self, device, enable=True):
        """Per-kernel HIP-event timing: False off, True every kernel, TIMING_K2 K2's events only."""
        _check(lib.pp_timing_enable(self.handle, device, int(enable)), "pp_timing_enable")

    def read_timing(self, device):
        """(ms per kernel [k_prep, k_cand, k_winner], launches per kernel); clears the record."""
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        _check(lib.pp_timing_read(self.handle, device, ms, n), "pp_timing_read")
        return list(ms), list(n)

    def close(self):
        if self.handle:
            lib.pp_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SCENE_FIELDS_F = ["ego_x", "ego_y", "ego_yaw_deg", "ego_speed_mph"]
SCENE_FIELDS_I = ["n_prev", "prev_target_lane", "n_cars"]
CAR_FIELDS_F = ["car_x", "car_y", "car_vx", "car_vy"]


def alloc_scenes(S, car_stride=12, xp="numpy", device=None):
    """SoA scene arrays (numpy on host, or torch on `device`)."""
    mk = _zeros(xp, device)
    d = {k: mk((S,), "f8") for k in SCENE_FIELDS_F}
    d.update({k: mk((S,), "i4") for k in SCENE_FIELDS_I})
    d["prev_x"] = mk((PREV_KEEP, S), "f8")
    d["prev_y"] = mk((PREV_KEEP, S), "f8")
    d["car_id"] = mk((car_stride, S), "i4")
    d.update({k: mk((car_stride, S), "f8") for k in CAR_FIELDS_F})
    return d


def scene_struct(d) -> SceneBatch:
    b = SceneBatch()
    b.n_scenes = int(d["ego_x"].shape[0])
    # (car arrays of None: a batch without car columns, car_stride = 0 and null pointers)
    b.car_stride = 0 if d["car_id"] is None else int(d["car_id"].shape[0])
    for k in SCENE_FIELDS_F + SCENE_FIELDS_I + CAR_FIELDS_F + ["prev_x", "prev_y", "car_id"]:
        setattr(b, k, _ptr(d[k]))
    for k in TABLE_FIELDS_I + TABLE_FIELDS_F:
        setattr(b, k, _ptr(d.get(k)))
    if d.get("tab_valid") is not None:
        b.tab_slots = int(d["tab_valid"].shape[0])
    return b


def add_car_table(d, slots=12, xp="numpy", device=None):
    """Adds the persistent car table (include/pp.h tab_*: `slots` slots per scene, slot j = id j,
    empty) to a scene dict."""
    S = int(d["ego_x"].shape[0])
    mk = _zeros(xp, device)
    for k in TABLE_FIELDS_I:
        d[k] = mk((slots, S), "i4")
    for k in TABLE_FIELDS_F:
        d[k] = mk((slots, S), "f8")
    for j in range(slots):
        d["tab_id"][j] = j
    return d


def alloc_traffic(S, n=12, xp="numpy", device=None):
    mk = _zeros(xp, device)
    return {"n_cars": 0, "lane": mk((n, S), "i4"), "seg": mk((n, S), "i4"), "t": mk((n, S), "f8"),
            "offset": mk((n, S), "f8"), "speed": mk((n, S), "f8")}


def traffic_struct(t) -> Traffic:
    T = _struct(Traffic, ["lane", "seg", "t", "offset", "speed"], t)
    T.n_cars = int(t["n_cars"])
    return T


def synth_traffic(m, S, seed=0x5EED0001, first=0, device=0, stream=None, car_stride=12):
    """Rollout start state on the GPU: (scenes with an empty car table, traffic)."""
    import torch
    dev = torch.device("cuda", device)
    d = add_car_table(alloc_scenes(S, car_stride, xp="torch", device=dev), xp="torch", device=dev)
    t = alloc_traffic(S, xp="torch", device=dev)
    b, T = scene_struct(d), traffic_struct(t)
    _check(lib.pp_synth_traffic(m.handle, seed, first, C.byref(b), C.byref(T), device, stream), "pp_synth_traffic")
    t["n_cars"] = T.n_cars
    return d, t


def synth_traffic_host(m, S, seed=0x5EED0001, first=0, car_stride=12, slots=12):
    d = add_car_table(alloc_scenes(S, car_stride), slots=slots)
    t = alloc_traffic(S)
    b, T = scene_struct(d), traffic_struct(t)
    _check(lib.pp_synth_traffic_host(m.handle, seed, first, C.byref(b), C.byref(T)), "pp_synth_traffic_host")
    t["n_cars"] = T.n_cars
    return d, t


def default_episode_cfg(**over) -> EpisodeCfg:
    """pp_episode_cfg_default, with fields overridden by keyword."""
    return _default_cfg(EpisodeCfg, lib.pp_episode_cfg_default, over)


def _episode_args(S, cfg, xp, device, judge, follow):
    cfg = cfg if cfg is not None else default_episode_cfg()
    n = max(int(cfg.n_cars), 1)
    if follow is not None:
        assert follow["desired"].shape[0] >= int(cfg.n_cars), "follow state holds fewer cars than the episode"
    d = add_car_table(alloc_scenes(S, max(n, 12), xp=xp, device=device), slots=max(n, 12), xp=xp, device=device)
    t = alloc_traffic(S, n=max(n, 12), xp=xp, device=device)
    J = judge_struct(judge) if judge is not None else None
    F = follow_struct(follow) if follow is not None else None
    return cfg, d, t, J, F


def synth_episode(m, S, seed=0x5EED0001, first=0, cfg=None, fcfg=None, device=0, stream=None, judge=None,
                  follow=None):
    """pp_synth_episode: a drivable start state on the GPU, (scenes with an empty car table, traffic).
    `judge` (alloc_judge) is made a warm state whose step numbers start at JUDGE_RING, `follow`
    (alloc_follow) is reset; fcfg: the gap rule (None: default_follow_cfg)."""
    import torch
    cfg, d, t, J, F = _episode_args(S, cfg, "torch", torch.device("cuda", device), judge, follow)
    b, T = scene_struct(d), traffic_struct(t)
    _check(lib.pp_synth_episode(m.handle, seed, first, _ref(cfg), _ref(fcfg), _ref(b), _ref(T), _ref(J), _ref(F),
                                device, stream), "pp_synth_episode")
    t["n_cars"] = T.n_cars
    return d, t


def synth_episode_host(m, S, seed=0x5EED0001, first=0, cfg=None, fcfg=None, judge=None, follow=None):
    """pp_synth_episode_host: synth_episode on the host (numpy arrays, the same bits)."""
    cfg, d, t, J, F = _episode_args(S, cfg, "numpy", None, judge, follow)
    b, T = scene_struct(d), traffic_struct(t)
    _check(lib.pp_synth_episode_host(m.handle, seed, first, _ref(cfg), _ref(fcfg), _ref(b), _ref(T), _ref(J),
                                     _ref(F)), "pp_synth_episode_host")
    t["n_cars"] = T.n_cars
    return d, t


def alloc_log(F, S, N=50, xp="numpy", device=None, plans=True):
    mk = _zeros(xp, device)
    lg = {k: mk((F, S), dt) for k, dt in LOG_FIELDS}
    if plans:
        lg["plan_x"] = mk((F, N, S), "f8")
        lg["plan_y"] = mk((F, N, S), "f8")
    return lg


def log_struct(lg) -> RolloutLog:
    return _struct(RolloutLog, [k for k, _ in LOG_FIELDS] + ["plan_x", "plan_y"], lg, optional=True)


def rollout(m, scenes, traffic, prm, result, n_frames, consume=3, sensor_range=300.0, log=None,
            device=0, stream=None):
    """pp_rollout: n_frames closed-loop frames on the GPU; scenes/traffic/result updated in place."""
    _rollout(lib.pp_rollout, "pp_rollout", m, scenes, traffic, prm, result, n_frames, consume, sensor_range, log,
             device, stream)


def _rollout(entry, what, m, scenes, traffic, prm, result, n_frames, consume, sensor_range, log, device, stream,
             *stages):
    """The four rollouts' call: their common arguments, then the entry point's own tail `stages`
    (configuration and state structures in its order; None: a null pointer)."""
    b, T, R = scene_struct(scenes), traffic_struct(traffic), result_struct(result)
    cfg = RolloutCfg(n_frames, consume, float(sensor_range))
    L = log_struct(log) if log is not None else None
    _check(entry(m.handle, _ref(b), _ref(T), _ref(prm), _ref(cfg), _ref(R), _ref(L), device, stream,
                 *[_ref(x) for x in stages]), what)


def _judge_stage(judge, jcfg):
    """(configuration, state structure) of a rollout's optional judge; a judge without a
    configuration gets the default one."""
    if judge is None:
        return jcfg, None
    return jcfg if jcfg is not None else default_judge_cfg(), judge_struct(judge)


def default_judge_cfg(**over) -> JudgeCfg:
    """pp_judge_cfg_default, with fields overridden by keyword."""
    return _default_cfg(JudgeCfg, lib.pp_judge_cfg_default, over)


def alloc_judge(S, xp="numpy", device=None):
    """Zero-filled judge state of S scenes (every scene a fresh episode)."""
    return _alloc_state(JUDGE_FIELDS, S, None, xp, device)


def judge_struct(j) -> Judge:
    return _struct(Judge, [k for k, _, _ in JUDGE_FIELDS], j)


def judge_to_numpy(j):
    out = _to_numpy(j)
    out["flags"] = out["flags"].view(np.uint32)
    return out


def judge_frame(m, scenes, traffic, result, judge, consume=3, cfg=None, host=None, device=0, stream=None):
    """pp_judge_frame / pp_judge_frame_host: judges the `consume` driven steps of one frame from the
    pre-frame scenes and traffic and the frame's plan; only `judge` is updated. host=None picks the
    host twin when the arrays are numpy."""
    if host is None:
        host = isinstance(scenes["ego_x"], np.ndarray)
    cfg = cfg if cfg is not None else default_judge_cfg()
    b, T, R, J = scene_struct(scenes), traffic_struct(traffic), result_struct(result), judge_struct(judge)
    if host:
        _check(lib.pp_judge_frame_host(m.handle, _ref(b), _ref(T), _ref(R), consume, _ref(cfg), _ref(J)),
               "pp_judge_frame_host")
    else:
        _check(lib.pp_judge_frame(m.handle, _ref(b), _ref(T), _ref(R), consume, _ref(cfg), _ref(J), device, stream),
               "pp_judge_frame")


def rollout_judged(m, scenes, traffic, prm, result, judge, n_frames, consume=3, sensor_range=300.0, log=None,
                   cfg=None, device=0, stream=None):
    """pp_rollout_judged: rollout() with the judge run on every frame; `judge` updated in place."""
    _rollout(lib.pp_rollout_judged, "pp_rollout_judged", m, scenes, traffic, prm, result, n_frames, consume,
             sensor_range, log, device, stream, cfg if cfg is not None else default_judge_cfg(), judge_struct(judge))


def default_follow_cfg(**over) -> FollowCfg:
    """pp_follow_cfg_default, with fields overridden by keyword."""
    return _default_cfg(FollowCfg, lib.pp_follow_cfg_default, over)


def alloc_follow(S, n=12, xp="numpy", device=None):
    """Zero-filled follow state of S scenes x n cars (every scene a fresh episode)."""
    return _alloc_state(FOLLOW_FIELDS, S, n, xp, device)


def follow_struct(f) -> Follow:
    return _struct(Follow, [k for k, _, _ in FOLLOW_FIELDS], f)


def follow_to_numpy(f):
    return _to_numpy(f)


def traffic_follow(m, scenes, traffic, follow, consume=3, cfg=None, host=None, device=0, stream=None):
    """pp_traffic_follow / pp_traffic_follow_host: the car-following update of one frame from the
    pre-frame scenes and traffic; traffic["speed"] and `follow` are updated in place. host=None picks
    the host twin when the arrays are numpy."""
    if host is None:
        host = isinstance(scenes["ego_x"], np.ndarray)
    cfg = cfg if cfg is not None else default_follow_cfg()
    assert follow["desired"].shape[0] >= int(traffic["n_cars"]), "follow state holds fewer cars than the traffic"
    b, T, F = scene_struct(scenes), traffic_struct(traffic), follow_struct(follow)
    if host:
        _check(lib.pp_traffic_follow_host(m.handle, _ref(b), _ref(T), consume, _ref(cfg), _ref(F)),
               "pp_traffic_follow_host")
    else:
        _check(lib.pp_traffic_follow(m.handle, _ref(b), _ref(T), consume, _ref(cfg), _ref(F), device, stream),
               "pp_traffic_follow")


def rollout_reactive(m, scenes, traffic, prm, result, follow, n_frames, consume=3, sensor_range=300.0, log=None,
                     judge=None, jcfg=None, fcfg=None, device=0, stream=None):
    """pp_rollout_reactive: rollout() whose traffic follows the vehicle ahead (follow state updated in
    place), judged on every frame when `judge` is given."""
    assert follow["desired"].shape[0] >= int(traffic["n_cars"]), "follow state holds fewer cars than the traffic"
    _rollout(lib.pp_rollout_reactive, "pp_rollout_reactive", m, scenes, traffic, prm, result, n_frames, consume,
             sensor_range, log, device, stream, *_judge_stage(judge, jcfg),
             fcfg if fcfg is not None else default_follow_cfg(), follow_struct(follow))


def default_lane_change_cfg(**over) -> LaneChangeCfg:
    """pp_lane_change_cfg_default, with fields overridden by keyword."""
    return _default_cfg(LaneChangeCfg, lib.pp_lane_change_cfg_default, over)


def alloc_lane_change(S, n=12, xp="numpy", device=None):
    """Zero-filled lane-change state of S scenes x n cars (every scene a fresh episode)."""
    return _alloc_state(LANE_CHANGE_FIELDS, S, n, xp, device)


def lane_change_struct(l) -> LaneChange:
    return _struct(LaneChange, [k for k, _, _ in LANE_CHANGE_FIELDS], l)


def lane_change_to_numpy(l):
    return _to_numpy(l)


def traffic_lane_change(m, scenes, traffic, follow, lane_change, consume=3, fcfg=None, cfg=None, host=None,
                        device=0, stream=None):
    """pp_traffic_lane_change / pp_traffic_lane_change_host: the lane changes of one frame, after
    traffic_follow of the same frame; traffic's lane, seg, t and offset and `lane_change` are updated in
    place. host=None picks the host twin when the arrays are numpy."""
    if host is None:
        host = isinstance(scenes["ego_x"], np.ndarray)
    fcfg = fcfg if fcfg is not None else default_follow_cfg()
    cfg = cfg if cfg is not None else default_lane_change_cfg()
    n = int(traffic["n_cars"])
    assert follow["desired"].shape[0] >= n, "follow state holds fewer cars than the traffic"
    assert lane_change["home"].shape[0] >= n, "lane-change state holds fewer cars than the traffic"
    b, T, F, L = scene_struct(scenes), traffic_struct(traffic), follow_struct(follow), lane_change_struct(lane_change)
    if host:
        _check(lib.pp_traffic_lane_change_host(m.handle, _ref(b), _ref(T), consume, _ref(fcfg), _ref(F), _ref(cfg),
                                               _ref(L)), "pp_traffic_lane_change_host")
    else:
        _check(lib.pp_traffic_lane_change(m.handle, _ref(b), _ref(T), consume, _ref(fcfg), _ref(F), _ref(cfg),
                                          _ref(L), device, stream), "pp_traffic_lane_change")


def rollout_lane_changing(m, scenes, traffic, prm, result, follow, lane_change, n_frames, consume=3,
                          sensor_range=300.0, log=None, judge=None, jcfg=None, fcfg=None, lcfg=None, device=0,
                          stream=None):
    """pp_rollout_lane_changing: rollout_reactive() whose traffic also changes lanes (lane-change state
    updated in place); lane_change=None: exactly rollout_reactive()."""
    n = int(traffic["n_cars"])
    assert follow["desired"].shape[0] >= n, "follow state holds fewer cars than the traffic"
    change = (None, None)         # (no lane-change state: no configuration either, whatever lcfg is)
    if lane_change is not None:
        assert lane_change["home"].shape[0] >= n, "lane-change state holds fewer cars than the traffic"
        change = (lcfg if lcfg is not None else default_lane_change_cfg(), lane_change_struct(lane_change))
    _rollout(lib.pp_rollout_lane_changing, "pp_rollout_lane_changing", m, scenes, traffic, prm, result, n_frames,
             consume, sensor_range, log, device, stream, *_judge_stage(judge, jcfg),
             fcfg if fcfg is not None else default_follow_cfg(), follow_struct(follow), *change)


def default_sensor_cfg(**over) -> SensorCfg:
    """pp_sensor_cfg_default (the identity sensor), with fields overridden by keyword."""
    return _default_cfg(SensorCfg, lib.pp_sensor_cfg_default, over)


def alloc_sensor(S, car_stride=12, xp="numpy", device=None):
    """Zero-filled sensor state of S scenes x car_stride rows (every scene a fresh episode)."""
    return _alloc_state(SENSOR_FIELDS, S, car_stride, xp, device)


def sensor_struct(x) -> Sensor:
    return _struct(Sensor, [k for k, _, _ in SENSOR_FIELDS], x)


def sensor_to_numpy(x):
    return _to_numpy(x)


def sensed_scenes(scenes, sensor):
    """The scene dict pp_eval is handed behind a sensor: `scenes` with the sensor state's rows in place
    of the truth's (the other arrays, the car table among them, shared)."""
    return dict(scenes, **{k: sensor[k] for k in SENSED_ROWS})


def sense_frame(scenes, sensor, cfg=None, host=None, device=0, stream=None):
    """pp_sense_frame / pp_sense_frame_host: one frame of the sensor model from the scenes' ego position
    and car rows (the truth, only read); `sensor` is updated in place. host=None picks the host twin
    when the arrays are numpy."""
    if host is None:
        host = isinstance(scenes["ego_x"], np.ndarray)
    cfg = cfg if cfg is not None else default_sensor_cfg()
    b = scene_struct(scenes)
    assert sensor["fate"].shape[0] >= b.car_stride, "sensor state holds fewer rows than the scenes' car_stride"
    X = sensor_struct(sensor)
    if host:
        _check(lib.pp_sense_frame_host(_ref(b), _ref(cfg), _ref(X)), "pp_sense_frame_host")
    else:
        _check(lib.pp_sense_frame(_ref(b), _ref(cfg), _ref(X), device, stream), "pp_sense_frame")


def rollout_sensed(m, scenes, traffic, prm, result, follow, lane_change, sensor, n_frames, consume=3,
                   sensor_range=300.0, log=None, judge=None, jcfg=None, fcfg=None, lcfg=None, scfg=None, device=0,
                   stream=None):
    """pp_rollout_sensed: rollout_lane_changing() whose planner sees the traffic through the sensor model
    (sensor state updated in place); everything else reads the truth. scfg=None: the identity sensor."""
    n = int(traffic["n_cars"])
    assert follow["desired"].shape[0] >= n, "follow state holds fewer cars than the traffic"
    assert sensor["fate"].shape[0] >= int(scenes["car_id"].shape[0]), "sensor state holds fewer rows than the scenes"
    change = (None, None)
    if lane_change is not None:
        assert lane_change["home"].shape[0] >= n, "lane-change state holds fewer cars than the traffic"
        change = (lcfg if lcfg is not None else default_lane_change_cfg(), lane_change_struct(lane_change))
    _rollout(lib.pp_rollout_sensed, "pp_rollout_sensed", m, scenes, traffic, prm, result, n_frames, consume,
             sensor_range, log, device, stream, *_judge_stage(judge, jcfg),
             fcfg if fcfg is not None else default_follow_cfg(), follow_struct(follow), *change,
             scfg if scfg is not None else default_sensor_cfg(), sensor_struct(sensor))


def default_tracker_cfg(**over) -> TrackerCfg:
    """pp_tracker_cfg_default (the identity tracker), with fields overridden by keyword."""
    return _default_cfg(TrackerCfg, lib.pp_tracker_cfg_default, over)


def alloc_tracker(S, car_stride=12, xp="numpy", device=None):
    """Zero-filled tracker state of S scenes x car_stride rows and 2 x car_stride track slots (every
    scene a fresh episode)."""
    return _alloc_state(TRACKER_FIELDS, S, car_stride, xp, device)


def tracker_struct(x) -> Tracker:
    return _struct(Tracker, [k for k, _, _ in TRACKER_FIELDS], x)


def tracker_to_numpy(x):
    return _to_numpy(x)


def tracked_scenes(scenes, tracker):
    """The scene dict pp_eval is handed behind a tracker: `scenes` with the tracker state's rows in place
    of its own (the other arrays, the car table among them, shared)."""
    return dict(scenes, **{k: tracker[k] for k in SENSED_ROWS})


def track_frame(seen, tracker, cfg=None, consume=3, host=None, device=0, stream=None):
    """pp_track_frame / pp_track_frame_host: one frame of the tracker from `seen`'s ego position and car
    rows (sensed_scenes(), or the plain truth; only read); `tracker` is updated in place. host=None picks
    the host twin when the arrays are numpy."""
    if host is None:
        host = isinstance(seen["ego_x"], np.ndarray)
    cfg = cfg if cfg is not None else default_tracker_cfg()
    b = scene_struct(seen)
    assert tracker["src"].shape[0] == b.car_stride and tracker["id"].shape[0] == 2 * b.car_stride, \
        "the tracker state's banks are laid out for another car_stride"
    X = tracker_struct(tracker)
    if host:
        _check(lib.pp_track_frame_host(_ref(b), _ref(cfg), consume, _ref(X)), "pp_track_frame_host")
    else:
        _check(lib.pp_track_frame(_ref(b), _ref(cfg), consume, _ref(X), device, stream), "pp_track_frame")


def rollout_tracked(m, scenes, traffic, prm, result, follow, lane_change, sensor, tracker, n_frames, consume=3,
                    sensor_range=300.0, log=None, judge=None, jcfg=None, fcfg=None, lcfg=None, scfg=None, tcfg=None,
                    device=0, stream=None):
    """pp_rollout_tracked: rollout_sensed() whose planner sees the sensed rows through the tracker
    (tracker state updated in place). sensor=None: the tracker works on the truth rows. tcfg=None: the
    identity tracker."""
    n, R = int(traffic["n_cars"]), int(scenes["car_id"].shape[0])
    assert follow["desired"].shape[0] >= n, "follow state holds fewer cars than the traffic"
    assert tracker["src"].shape[0] == R and tracker["id"].shape[0] == 2 * R, \
        "the tracker state's banks are laid out for another car_stride"
    change, sense = (None, None), (None, None)
    if lane_change is not None:
        assert lane_change["home"].shape[0] >= n, "lane-change state holds fewer cars than the traffic"
        change = (lcfg if lcfg is not None else default_lane_change_cfg(), lane_change_struct(lane_change))
    if sensor is not None:
        assert sensor["fate"].shape[0] >= R, "sensor state holds fewer rows than the scenes"
        sense = (scfg if scfg is not None else default_sensor_cfg(), sensor_struct(sensor))
    _rollout(lib.pp_rollout_tracked, "pp_rollout_tracked", m, scenes, traffic, prm, result, n_frames, consume,
             sensor_range, log, device, stream, *_judge_stage(judge, jcfg),
             fcfg if fcfg is not None else default_follow_cfg(), follow_struct(follow), *change, *sense,
             tcfg if tcfg is not None else default_tracker_cfg(), tracker_struct(tracker))


def alloc_judge_stats(rows, bins=64, xp="numpy", device=None):
    """Zero arrays for `rows` rows of summary figures with a histogram of `bins` bins (pp_judge_stats)."""
    mk = _zeros(xp, device)
    return {k: mk((rows,) if lead is None else (bins if lead == "b" else lead, rows), dt)
            for k, dt, lead in STATS_FIELDS}


def stats_struct(st) -> JudgeStats:
    return _struct(JudgeStats, [k for k, _, _ in STATS_FIELDS], st)


def stats_to_numpy(st):
    return _to_numpy(st)


HIST_MAX_DEFAULT = 2000.0      # metres: above what 4,000 driven steps at the speed limit cover


def judge_summary(judge, S, scenes_per_group=None, hist_bins=64, hist_max=HIST_MAX_DEFAULT, host=None, device=0,
                  stream=None, m=None, stats=None, out_first=0):
    """pp_judge_summary / pp_judge_summary_host: one row of figures per group of `scenes_per_group`
    scenes (None: S, one row) of the judge state's first S scenes; returns the dict of arrays
    (alloc_judge_stats). host=None picks the host twin when the arrays are numpy; the device call
    needs the map `m`, whose stream workspace holds the tile partials. `stats`: write rows out_first..
    of these arrays (they hold stats["n_scenes"].shape[0] rows) and leave the others alone."""
    if host is None:
        host = isinstance(judge["steps"], np.ndarray)
    E = S if scenes_per_group is None else scenes_per_group
    G = -(-S // E) if E >= 1 else 0
    if stats is None:
        if host:
            stats = alloc_judge_stats(G, hist_bins)
        else:
            import torch
            stats = alloc_judge_stats(G, hist_bins, xp="torch", device=torch.device("cuda", device))
        stride = 0
    else:
        assert stats["hist"].shape[0] >= hist_bins, "stats hold fewer bins than hist_bins"
        stride = int(stats["n_scenes"].shape[0])
    cfg = SummaryCfg(E, hist_bins, 0, float(hist_max), out_first, stride)
    J, O = judge_struct(judge), stats_struct(stats)
    if host:
        _check(lib.pp_judge_summary_host(_ref(J), S, _ref(cfg), _ref(O)), "pp_judge_summary_host")
    else:
        if m is None:
            raise ValueError("judge_summary on the device needs the map m")
        _check(lib.pp_judge_summary(m.handle, _ref(J), S, _ref(cfg), _ref(O), device, stream), "pp_judge_summary")
    return stats


def stats_quantile(stats, row, q, hist_max=HIST_MAX_DEFAULT):
    """(lo, hi): the edges of the first histogram bin of `row` whose cumulative count reaches
    ceil(q n), n the histogram's total; the clean_dist of rank ceil(q n) lies in [lo, hi) (the last
    bin: hi = +inf, it also holds everything beyond hist_max). (nan, nan) for an empty histogram."""
    import math
    h = stats["hist"]
    h = (h if isinstance(h, np.ndarray) else h.cpu().numpy())[:, row]
    B, n = len(h), int(h.sum())
    if n == 0:
        return float("nan"), float("nan")
    need = max(1, math.ceil(q * n))
    b = int(np.searchsorted(np.cumsum(h), need))
    inv_w = B / float(hist_max)

    def edge(k):
        # the kernel's bin is (int)(x * inv_w): bin k starts at the smallest x with x * inv_w >= k,
        # which lies within a few ulps of k / inv_w (the product is monotone in x)
        x = k / inv_w
        while x * inv_w < k:
            x = math.nextafter(x, math.inf)
        while x > 0 and math.nextafter(x, -math.inf) * inv_w >= k:
            x = math.nextafter(x, -math.inf)
        return x

    return edge(b), (math.inf if b == B - 1 else edge(b + 1))


def rollout_sweep(m, sets, S, n_frames, scenes_per_group=None, seed=0x5EED0001, first=0, consume=3,
                  sensor_range=300.0, hist_bins=64, hist_max=HIST_MAX_DEFAULT, ecfg=None, jcfg=None, fcfg=None,
                  lcfg=None, lane_changes=True, device=0, stream=None, buffers=None, sensors=None, sensor=None,
                  trackers=None, tracker=None):
    """pp_rollout_sweep: drives the same S seeded episodes (synth_episode) once per parameter set of
    `sets` (a list of Params) through rollout_lane_changing and summarises each drive per group of
    `scenes_per_group` scenes (None: S), all on the one stream with no host synchronisation. Returns
    (stats, buffers): the dict of device arrays of len(sets) * G rows, set p's group g in row p * G +
    g, and the drive's buffers (scenes, traffic, result, judge, follow, lane_change: the last set's end
    state), which a later call of the same sizes may pass back in. `sensors` (a list of SensorCfg, one per
    set): pp_rollout_sweep_sensed, set p driven through rollout_sensed with sensors[p]; `sensor` is its
    state (None: allocated; buffers["sensor"] either way). `trackers` (a list of TrackerCfg, one per
    set; sensors=None: identity sensors): pp_rollout_sweep_tracked, set p driven through rollout_tracked
    with sensors[p] and trackers[p]; `tracker` is its state (buffers["tracker"])."""
    import torch
    dev = torch.device("cuda", device)
    ecfg = ecfg if ecfg is not None else default_episode_cfg()
    jcfg = jcfg if jcfg is not None else default_judge_cfg()
    fcfg = fcfg if fcfg is not None else default_follow_cfg()
    E = S if scenes_per_group is None else scenes_per_group
    G = -(-S // E) if E >= 1 else 0
    P = len(sets)
    n = max(int(ecfg.n_cars), 12)
    if buffers is None:
        big = default_params(n_speeds=max([int(p.n_speeds) for p in sets] + [1]),
                             n_points=max([int(p.n_points) for p in sets] + [1]))
        buffers = {"scenes": add_car_table(alloc_scenes(S, n, xp="torch", device=dev), slots=n, xp="torch", device=dev),
                   "traffic": alloc_traffic(S, n=n, xp="torch", device=dev),
                   "result": alloc_result(S, big, xp="torch", device=dev),
                   "judge": alloc_judge(S, xp="torch", device=dev),
                   "follow": alloc_follow(S, n=n, xp="torch", device=dev),
                   "lane_change": alloc_lane_change(S, n=n, xp="torch", device=dev) if lane_changes else None}
    lc = buffers.get("lane_change")
    L = lane_change_struct(lc) if lc is not None else None
    if lc is not None and lcfg is None:
        lcfg = default_lane_change_cfg()
    stats = alloc_judge_stats(P * G, hist_bins, xp="torch", device=dev)
    arr = (Params * max(P, 1))(*sets)
    cfg = SweepCfg(P, 0, seed, first, RolloutCfg(n_frames, consume, float(sensor_range)),
                   SummaryCfg(E, hist_bins, 0, float(hist_max), 0, 0))
    b, T, R = scene_struct(buffers["scenes"]), traffic_struct(buffers["traffic"]), result_struct(buffers["result"])
    J, F, O = judge_struct(buffers["judge"]), follow_struct(buffers["follow"]), stats_struct(stats)
    args = (m.handle, arr, _ref(cfg), _ref(ecfg), _ref(jcfg), _ref(fcfg), _ref(lcfg) if lc is not None else None,
            _ref(b), _ref(T), _ref(R), _ref(J), _ref(F), _ref(L), _ref(O), device, stream)
    if trackers is not None and sensors is None:
        sensors = [default_sensor_cfg() for _ in range(P)]
    if sensors is None:
        _check(lib.pp_rollout_sweep(*args), "pp_rollout_sweep")
    else:
        assert len(sensors) == P, "one sensor per parameter set"
        if sensor is None:
            sensor = buffers.get("sensor")
        if sensor is None:
            sensor = alloc_sensor(S, int(buffers["scenes"]["car_id"].shape[0]), xp="torch", device=dev)
        buffers["sensor"] = sensor
        sarr = (SensorCfg * max(P, 1))(*sensors)
        if trackers is None:
            _check(lib.pp_rollout_sweep_sensed(*args, sarr, _ref(sensor_struct(sensor))), "pp_rollout_sweep_sensed")
        else:
            assert len(trackers) == P, "one tracker per parameter set"
            if tracker is None:
                tracker = buffers.get("tracker")
            if tracker is None:
                tracker = alloc_tracker(S, int(buffers["scenes"]["car_id"].shape[0]), xp="torch", device=dev)
            buffers["tracker"] = tracker
            tarr = (TrackerCfg * max(P, 1))(*trackers)
            _check(lib.pp_rollout_sweep_tracked(*args, sarr, _ref(sensor_struct(sensor)), tarr,
                                                _ref(tracker_struct(tracker))), "pp_rollout_sweep_tracked")
    buffers["traffic"]["n_cars"] = int(ecfg.n_cars)
    return stats, buffers


def plan_reset(m, device=0):
    _check(lib.pp_plan_reset(m.handle, device), "pp_plan_reset")


def scenes_to_numpy(d):
    return _to_numpy(d)


def synth_host(m: Map, S, seed=0x5EED0001, first=0, car_stride=12):
    d = alloc_scenes(S, car_stride)
    b = scene_struct(d)
    _check(lib.pp_synth_scenes_host(m.handle, seed, first, C.byref(b)), "pp_synth_scenes_host")
    return d


def synth_device(m: Map, S, seed=0x5EED0001, first=0, device=0, stream=None, car_stride=12):
    import torch
    d = alloc_scenes(S, car_stride, xp="torch", device=torch.device("cuda", device))
    b = scene_struct(d)
    _check(lib.pp_synth_scenes(m.handle, seed, first, C.byref(b), device, stream), "pp_synth_scenes")
    return d


def alloc_result(S, prm: Params, xp="numpy", device=None, info=False):
    D = max(prm.n_draws, 1)
    Cn = D * NUM_LANES * prm.n_speeds
    N = prm.n_points
    mk = _zeros(xp, device)
    # next_x/next_y are point-major [N][S] (include/pp.h)
    r = {"winner": mk((S,), "i4"), "n_out": mk((S,), "i4"), "next_x": mk((N, S), "f8"),
         "next_y": mk((N, S), "f8"), "cost": mk((S, Cn), "f8"), "status": mk((S,), "u4")}
    if prm.emit_paths:
        r["paths"] = mk((S, N, Cn, 2), "f8")
        r["path_len"] = mk((S, Cn), "i4")
    if D > 1:
        r["draw_mean_cost"] = mk((S, NUM_LANES * prm.n_speeds), "f8")
    if info:
        if xp == "numpy":
            r["info"] = np.zeros((S,), INFO_DTYPE)
        else:
            import torch
            r["info"] = torch.zeros((S, INFO_DTYPE.itemsize), dtype=torch.uint8, device=device)
    return r


def result_struct(r) -> Result:
    return _struct(Result, ["winner", "n_out", "next_x", "next_y", "cost", "status", "paths", "path_len", "info",
                            "draw_mean_cost"], r, optional=True)


def result_to_numpy(r):
    out = {}
    for k, v in r.items():
        a = v if isinstance(v, np.ndarray) else v.cpu().numpy()
        if k == "status":
            a = a.view(np.uint32)
        if k == "info" and a.dtype == np.uint8:
            a = a.view(INFO_DTYPE).reshape(-1)
        out[k] = a
    return out


def evaluate(m: Map, scenes, prm: Params, result, device=0, stream=None):
    """pp_eval over device-resident scene/result buffers (torch tensors on cuda:device)."""
    b = scene_struct(scenes)
    R = result_struct(result)
    _check(lib.pp_eval(m.handle, C.byref(b), C.byref(prm), C.byref(R), device, stream), "pp_eval")


def plan_frame(m: Map, ego_x, ego_y, ego_yaw_deg, ego_speed_mph, prev_x, prev_y, cars,
               target_lane=1, device=0):
    """The onMessage replacement (src/main.cpp:1229-1466) for one telemetry frame.

    cars: iterable of (id, x, y, vx, vy[, s, d]) rows, as in the simulator's sensor_fusion.
    Returns (next_x, next_y, new_target_lane).
    """
    px = np.ascontiguousarray(prev_x, np.float64)
    py = np.ascontiguousarray(prev_y, np.float64)
    rows = [tuple(r)[:5] for r in cars]
    ids = np.array([int(r[0]) for r in rows], np.int32)
    cx = np.array([r[1] for r in rows], np.float64)
    cy = np.array([r[2] for r in rows], np.float64)
    cvx = np.array([r[3] for r in rows], np.float64)
    cvy = np.array([r[4] for r in rows], np.float64)
    tl = C.c_int32(target_lane)
    nx = np.zeros(50, np.float64)
    ny = np.zeros(50, np.float64)
    n_out = C.c_int32(0)
    _check(lib.pp_plan_frame(m.handle, device, ego_x, ego_y, ego_yaw_deg, ego_speed_mph,
                             px.ctypes.data_as(_dp), py.ctypes.data_as(_dp), len(px),
                             ids.ctypes.data_as(_ip), cx.ctypes.data_as(_dp),
                             cy.ctypes.data_as(_dp), cvx.ctypes.data_as(_dp),
                             cvy.ctypes.data_as(_dp), len(rows), C.byref(tl),
                             nx.ctypes.data_as(_dp), ny.ctypes.data_as(_dp), C.byref(n_out)),
           "pp_plan_frame")
    n = n_out.value
    return nx[:n].copy(), ny[:n].copy(), tl.value


DATA_DIR = os.path.join(os.path.dirname(_HERE), "data")


# pp_timing_enable modes (include/pp.h PP_TIMING_*)
TIMING_ALL, TIMING_K2 = 1, 2

# pp_debug_set keys and launch shapes (include/pp.h PP_DBG_*, PP_SHAPE_*)
DBG_PREP_GROUP, DBG_PREP_WAVES, DBG_SHAPE, DBG_POISON, DBG_SPLIT, DBG_LAST_PARTS, DBG_SORT_CARS = 0, 1, 2, 3, 4, 5, 6
DBG_PERSIST, DBG_LAST_PERSIST, DBG_LAST_PERSIST_SHAPE = 7, 8, 9
SPLIT_AUTO, SPLIT_ON, SPLIT_OFF = 0, 1, 2
PERSIST_AUTO, PERSIST_ON, PERSIST_OFF = 0, 1, 2
SHAPE_AUTO, SHAPE_SPLIT, SHAPE_CAND_SMALL, SHAPE_STEP = 0, 1, 2, 3


def debug_set(key, value):
    """Process-wide debug switch of the library (pp_debug_set; 0 = the library's own choice)."""
    _check(lib.pp_debug_set(key, value), "pp_debug_set")


def debug_get(key):
    return lib.pp_debug_get(key)


class debug:
    """Context manager: `with ppamd.debug(ppamd.DBG_SHAPE, ppamd.SHAPE_SPLIT): ...` sets a debug
    switch and restores its previous value on exit."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.prev = debug_get(self.key)
        debug_set(self.key, self.value)
        return self

    def __exit__(self, *exc):
        debug_set(self.key, self.prev)
        return False


def set_prep_group(lanes):
    """K1 lanes per evaluation (1, 2, 4, 8, 16; 0 = automatic): pp_debug_set(PP_DBG_PREP_GROUP)."""
    debug_set(DBG_PREP_GROUP, lanes)


def highway_map():
    """x, y of the reference's data/highway_map.csv (the only columns the path reads,
    src/main.cpp:1181-1193), stored as float64 in data/highway_map.npz."""
    z = np.load(os.path.join(DATA_DIR, "highway_map.npz"))
    return z["x"].copy(), z["y"].copy()


def version() -> str:
    return lib.pp_version().decode()


LIBM_KINDS = {"sin": 0, "cos": 1, "atan2": 2}


def libm_eval(kind, a, b=None, device=None):
    """pp_libm_eval: the kernels' restated glibc sin/cos/atan2 (csrc/pp_glibcm.h) over a float64
    array; numpy arrays run the host build, torch CUDA tensors the device build."""
    k = LIBM_KINDS[kind]
    if device is None:
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b if b is not None else a, np.float64)
        out = np.empty_like(a)
        _check(lib.pp_libm_eval(k, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size, -1, None), "pp_libm_eval")
        return out
    import torch
    b = b if b is not None else a
    out = torch.empty_like(a)
    st = torch.cuda.current_stream(device).cuda_stream
    _check(lib.pp_libm_eval(k, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), device, st), "pp_libm_eval")
    return out


# include/pp.h PP_MATH_*: kind -> (number, inputs, outputs)
MATH_KINDS = {name: (i, nin, nout) for i, (name, nin, nout) in enumerate([
    ("sincos", 1, 2), ("sincos_nolarge", 1, 2), ("atan2_pp", 2, 1), ("atan2_fast", 2, 1), ("atan2_unit", 2, 1),
    ("asin_small", 1, 1), ("rcp_nr", 1, 1), ("div_rcp", 3, 1), ("div_rcp_nc", 3, 1), ("div_rcp_auto", 2, 1),
    ("div_rcp_nc_auto", 2, 1), ("div50", 1, 1), ("div50_nc", 1, 1), ("sqrt_rd", 1, 3), ("div_rcp_n", 2, 1),
    ("div_rcp_d", 2, 1), ("fmod_2pi", 1, 1), ("fmod_2pi_small", 1, 1), ("turn_sincos", 1, 2),
    ("turn_sincos_nolarge", 1, 2), ("sincos_small", 1, 2), ("turn_angle", 3, 1), ("turn_angle_nolarge", 3, 1),
    ("turn_angle_fast", 3, 1), ("sc_speed", 4, 1), ("sc_speed_r", 4, 1), ("sc_speed_r_nc", 4, 1),
    ("sc_override", 4, 1), ("sc_override_r", 4, 1), ("sc_override_r_nc", 4, 1), ("speed_in_range", 1, 1)])}


def math_eval(kind, a, b=None, c=None, d=None, device=0):
    """pp_math_eval: one of the candidate loop's FP64 primitives (csrc/pp_math.h and its wrappers)
    over float64 torch tensors on `device`; returns the tuple of the kind's outputs, each of a's
    shape. For the sc_* kinds d is [2, n] (shift, step count k; t = 0.02 k) or, for sc_override*,
    [3, n] (shift, k, speed)."""
    import torch
    k, nin, nout = MATH_KINDS[kind]
    ins = [a, b, c, d]
    if any(x is None for x in ins[:nin]):
        raise ValueError(f"math_eval({kind}) takes {nin} inputs")
    ins = [x.contiguous() if x is not None else None for x in ins]
    n = ins[0].numel()
    dplanes = 3 if kind.startswith("sc_override") else 2
    for j, x in enumerate(ins[:nin]):
        planes = dplanes if j == 3 else 1
        if x.dtype != torch.float64 or not x.is_cuda or x.numel() != planes * n:
            raise ValueError(f"math_eval({kind}): input {j} must be a float64 device tensor of {planes} x {n}")
    outs = [torch.empty_like(ins[0]) for _ in range(nout)]
    st = torch.cuda.current_stream(device).cuda_stream
    p = [x.data_ptr() if x is not None else None for x in ins[:nin]] + [None] * (4 - nin)
    o = [x.data_ptr() for x in outs] + [None] * (3 - nout)
    _check(lib.pp_math_eval(k, *p, *o, n, device, st), "pp_math_eval")
    return tuple(outs)


# ---- wire codec (include/pp.h pp_telemetry_parse / pp_control_format; host) ----------------------
def pack_messages(msgs):
    """list of bytes -> (contiguous buffer, int64 offsets[n + 1])"""
    off = np.zeros(len(msgs) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return b"".join(msgs), off


def telemetry_parse(msgs, car_stride=MAX_CARS, threads=8):
    """Socket.io telemetry frames -> (host scene dict, per-message status)."""
    buf, off = pack_messages(msgs)
    n = len(msgs)
    d = alloc_scenes(n, car_stride)
    st = np.zeros(n, np.int32)
    b = scene_struct(d)
    _check(lib.pp_telemetry_parse(buf, off.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(b),
                                  st.ctypes.data_as(C.POINTER(C.c_int32)), threads), "pp_telemetry_parse")
    return d, st


def control_format(next_x, next_y, n_out, threads=8):
    """Point-major host next_x/next_y [N][S] + n_out -> list of control messages (bytes)."""
    nx = np.ascontiguousarray(next_x, np.float64)
    ny = np.ascontiguousarray(next_y, np.float64)
    no = np.ascontiguousarray(n_out, np.int32)
    S = no.shape[0]
    off = np.zeros(S + 1, np.int64)
    cap = max(1024, S * 2048)
    while True:
        out = C.create_string_buffer(cap)
        rc = lib.pp_control_format(nx.ctypes.data_as(_dp), ny.ctypes.data_as(_dp),
                                   no.ctypes.data_as(C.POINTER(C.c_int32)), S, nx.shape[-1] if nx.ndim > 1 else S,
                                   out, cap, off.ctypes.data_as(C.POINTER(C.c_int64)), threads)
        if rc == -3:
            cap = int(off[-1]) + 1
            continue
        _check(rc, "pp_control_format")
        raw = out.raw
        return [raw[off[i]:off[i + 1]] for i in range(S)]


def plan_batch_host(m, scenes, prm, device=0):
    """pp_plan_batch_host: host scene dict (optionally with a car table, updated in place) ->
    host result dict (winner, n_out, next_x/next_y [N][S], cost, status)."""
    S = int(scenes["ego_x"].shape[0])
    r = alloc_result(S, prm)
    _check(lib.pp_plan_batch_host(m.handle, device, C.byref(scene_struct(scenes)), C.byref(prm),
                                  C.byref(result_struct(r)), None), "pp_plan_batch_host")
    return r


class Server:
    """pp_serve on a background thread (ctypes releases the GIL for the blocking call)."""

    def __init__(self, m, port=0, max_clients=64, n_speeds=1, threads=4, device=0, max_frames=0):
        import threading
        self.m = m
        self.opts = ServerOpts(b"127.0.0.1", port, max_clients, n_speeds, threads, device, 0, max_frames)
        self.stop_flag = C.c_int32(0)
        self.port = C.c_int32(0)
        self.stats = (C.c_int64 * 4)()
        self.rc = None
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        import time
        t0 = time.time()
        while self.port.value == 0 and self.rc is None and time.time() - t0 < 10:
            time.sleep(0.005)
        if self.port.value == 0:
            raise PPError(f"pp_serve did not start (rc={self.rc})")

    def _run(self):
        self.rc = lib.pp_serve(self.m.handle, C.byref(self.opts), C.byref(self.stop_flag), C.byref(self.port),
                               self.stats)

    def close(self):
        self.stop_flag.value = 1
        self.thread.join(timeout=30)
        return self.rc, list(self.stats)


MSG_HOST = 4                      # device codec: the frame needs the host codec


def upload_messages(msgs, device=0):
    """Frames -> (16-byte aligned padded uint8 device buffer, int64 device offsets)."""
    import torch
    buf, off = pack_messages(msgs)
    n = (len(buf) + 15) // 16 * 16 + 16
    host = np.zeros(n, np.uint8)
    host[:len(buf)] = np.frombuffer(buf, np.uint8)
    dev = torch.device("cuda", device)
    return torch.from_numpy(host).to(dev), torch.from_numpy(off).to(dev)


def telemetry_parse_device(msgs, car_stride=MAX_CARS, device=0, stream=None, d_buf=None, d_off=None):
    """pp_telemetry_parse_device -> (device scene dict, device status)."""
    import torch
    dev = torch.device("cuda", device)
    if d_buf is None:
        d_buf, d_off = upload_messages(msgs, device)
    n = int(d_off.shape[0]) - 1
    d = alloc_scenes(n, car_stride, xp="torch", device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    b = scene_struct(d)
    _check(lib.pp_telemetry_parse_device(d_buf.data_ptr(), d_off.data_ptr(), n, C.byref(b), st.data_ptr(), device,
                                         stream), "pp_telemetry_parse_device")
    return d, st


def control_format_device(next_x, next_y, n_out, slot_bytes=2560, device=0, stream=None):
    """pp_control_format_device on torch [N][S] tensors -> (slots uint8 [S, slot_bytes], len int32 [S])."""
    import torch
    S = int(n_out.shape[0])
    slots = torch.empty((S, slot_bytes), dtype=torch.uint8, device=next_x.device)
    ln = torch.empty(S, dtype=torch.int32, device=next_x.device)
    _check(lib.pp_control_format_device(next_x.data_ptr(), next_y.data_ptr(), n_out.data_ptr(), S,
                                        int(next_x.shape[-1]), slots.data_ptr(), slot_bytes, ln.data_ptr(), device,
                                        stream), "pp_control_format_device")
    return slots, ln


def slots_to_messages(slots, lens):
    """Host copies of device slots -> list of bytes (None where the host codec must format)."""
    sl = slots if isinstance(slots, np.ndarray) else slots.cpu().numpy()
    ln = lens if isinstance(lens, np.ndarray) else lens.cpu().numpy()
    return [bytes(sl[i, :ln[i]]) if ln[i] >= 0 else None for i in range(len(ln))]
