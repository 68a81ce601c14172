// pp_eval.hip — MI355X (gfx950) batched trajectory-candidate evaluator + its C-ABI.
//
// Pipeline per pp_eval call:
//   K1 k_prep    one lane per scene, map staged in LDS: ego derivation, Frenet frame, car matching,
//                LaneChangePlanner, follow cars + LimitSpeed per candidate lane
//                (src/main.cpp:1254-1438) -> per-scene prep record (SoA workspace).
//   K2 k_cand    one workgroup = SPB scenes x C candidates. Phase A: one lane per (scene, lane)
//                builds the control points + tk::spline coefficients into LDS
//                (TrajectoryBuilder::build setup, src/main.cpp:575-904, spline.h:284-373).
//                Phase B: one lane per candidate runs the 0.02 s resampling loop with the
//                accel/curvature limiter (src/main.cpp:905-1041) reading its spline from LDS
//                and computes the candidate cost (cost-only loop unless every path is emitted).
//   K3 k_winner  comfort mode: per-scene argmin + re-run of the winning candidate with outputs.
//                (reference mode: the winner is known before the loop; k_cand's first wave of
//                each block runs the winners and writes next_x/next_y)
//
// This file is the evaluator's one translation unit and holds no code of its own: the headers
// included below are its parts, in order. Device side: diagnostic-build hooks (pp_diag.h); the
// output frame, winner record and map staging (pp_k_frame.h); K0/K1 scene preparation
// (pp_k_prep.h); phase A's spline slots (pp_k_spline.h); K2 candidates (pp_k_cand.h); K3/K4 output
// (pp_k_out.h); the fused small-batch and frame kernels (pp_k_step.h); rollout, synthesis, map and
// libm kernels (pp_k_world.h); the primitives' test kernel (pp_k_math.h). Then the host side: maps,
// device resources and the world stages' tables and per-scene launch (pp_host_map.h), pp_eval's
// launches (pp_launch.h), the C ABI (pp_api.h, pp_api_rollout.h, pp_api_frame.h). The world stages'
// shared arithmetic and default configurations are pp_judge.h, pp_follow.h, pp_lanechange.h, pp_episode.h;
// the judge summary's is pp_summary.h, the sensor model's pp_sensor.h, the tracker's pp_tracker.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/pp.h"
#include "pp_cartable.h"
#include "pp_diag.h"         // the diagnostic builds' hooks (empty macros in the product build)
#include "pp_device.h"
#include "pp_glibcm.h"
#include "pp_math.h"
#include "pp_synth.h"
#include "pp_judge.h"
#include "pp_follow.h"
#include "pp_lanechange.h"
#include "pp_episode.h"
#include "pp_summary.h"
#include "pp_sensor.h"
#include "pp_tracker.h"

using namespace ppd;

#include "pp_k_frame.h"      // map view, output frame, tunables, winner record, map staging
#include "pp_k_prep.h"       // K0/K1: k_sort_cars, k_prep, k_prep_g2..16
#include "pp_k_spline.h"     // phase A: Slot, setup_lane, team_a1..a5
#include "pp_k_cand.h"       // K2: run_candidate, cand_group, k_cand
#include "pp_k_out.h"        // K3/K4: k_winner, k_winner_st, k_emit
#include "pp_k_step.h"       // k_cand_small, k_step_small(512), k_plan_frame
#include "pp_k_world.h"      // k_sim, k_judge, k_follow, k_lane_change, k_sense, k_track, k_summary_*, k_synth*, map kernels, k_libm
#include "pp_k_math.h"       // k_math: the loop's FP64 primitives over arrays (pp_math_eval)

// ================================================================================================
// host side (one translation unit with the kernels above, so the launches see them)
// ================================================================================================
#include "pp_host_map.h"     // pp_map, DevState, StreamWS, build_map, dev_init, WorldDev, launch_scenes
#include "pp_launch.h"       // workspace, launch-shape choices, eval_impl and its launch sequences
#include "pp_api.h"          // C ABI: params, maps, reserve, pp_eval, debug, timing, synthesis, diagnostics
#include "pp_api_rollout.h"  // C ABI: rollouts, judge, follow, lane change, summary, sweep, sensor, tracker
#include "pp_api_frame.h"    // C ABI: pp_plan_batch_host, pp_plan_reset, pp_plan_frame
