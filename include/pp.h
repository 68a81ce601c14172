/*
 * pp.h — C-ABI of the MI355X batched trajectory-candidate evaluator.
 *
 * This header is the drop-in boundary. It replaces the reference's per-frame websocket glue
 * (Fable3/CarND-Path-Planning-Project, src/main.cpp:1214-1474: the uWS `onMessage` lambda that
 * parses telemetry, runs the planner and replies with next_x/next_y) by a batch interface:
 * many scenes in, per-candidate costs + one winning next_x/next_y path per scene out.
 *
 *   reference interface                         replaced by
 *   ------------------------------------------  -----------------------------------------------
 *   main(): CSV load + Map::Init                pp_map_create / pp_map_destroy
 *     (src/main.cpp:1160-1193, 89-131)
 *   onMessage compute body (src/main.cpp:       pp_eval (batched, device-resident SoA buffers)
 *     1229-1457) for ONE telemetry frame        pp_plan_frame (one frame, host buffers — the
 *                                                 literal onMessage replacement, C = 1)
 *   TrajectoryBuilder::build (src/main.cpp:     every candidate (lane, speed) of pp_eval runs this
 *     565-1049)                                   exact algorithm; see DESIGN.md
 *
 * Plain C: no torch or HIP types cross this boundary. Device pointers are `void*`/typed pointers
 * into HIP device memory (hipMalloc, or torch tensors' data_ptr()). Every entry point returns an
 * int32 status (PP_OK = 0, negative on error) and never throws.
 */
#ifndef PP_H
#define PP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fixed sizes ------------------------------------------------------------------------- */
#ifndef PP_NUM_LANES        /* src/main.cpp:22 NUM_LANES (a build-time constant there too; the */
#define PP_NUM_LANES   3    /* library is built for one value: pp_num_lanes() reports it)      */
#endif
#define PP_PREV_KEEP   10   /* src/main.cpp:1258 prev_trajectory_length                       */
/* sensor_fusion rows per scene and car-table slots (the simulator reports 12; the reference's
 * std::map<int, Car> has no bound, src/main.cpp:1194): 256 for up to three lanes, 64 beyond (the
 * planner's order-dependent minima carry each winner's iteration index in a 64-bit word) */
#if PP_NUM_LANES <= 3
#define PP_MAX_CARS    256
#else
#define PP_MAX_CARS    64
#endif
/* the Monte-Carlo noise counter's car stride (pp_mc_gauss): fixed, so a seed draws the same noise
 * in every build whatever its PP_MAX_CARS (which never exceeds it) */
#define PP_NOISE_CAR_STRIDE 256
#define PP_MAX_SPEEDS  8    /* target speeds per lane                                          */
#define PP_MAX_POINTS  128  /* horizon N upper bound (reference: 50, src/main.cpp:854,1039)   */
#define PP_MAX_KNOTS   16   /* spline knots: 9 prev + 1 + 5 control points (src/main.cpp:744) */
#define PP_MAX_DRAWS   1024 /* Monte-Carlo sensor-noise draws per scene (pp_params.n_draws)   */

/* ---- status codes ------------------------------------------------------------------------ */
#define PP_OK              0
#define PP_ERR_ARG        -1   /* null pointer / out-of-range size                              */
#define PP_ERR_HIP        -2   /* HIP runtime error                                            */
#define PP_ERR_NOMEM      -3
#define PP_ERR_NODEVICE   -4
#define PP_ERR_STATE      -5   /* PP_DBG_POISON: a device buffer was not in its between-calls state */

/* ---- per-scene status flags (pp_result.status) -------------------------------------------- */
#define PP_ST_EGO_UNMATCHED  (1u << 0)  /* src/main.cpp:1302-1307 "can't lane match ego"        */
#define PP_ST_CAR_UNMATCHED  (1u << 1)  /* src/main.cpp:1336-1340 car erased                    */
#define PP_ST_FALLBACK       (1u << 2)  /* some candidate used the fallback integrator :848     */
#define PP_ST_SPLINE_TRUNC   (1u << 3)  /* some candidate truncated non-monotone knots :833     */
#define PP_ST_NAN            (1u << 4)  /* some candidate produced a NaN cost / bounded walk hit */
#define PP_ST_COLLISION      (1u << 5)  /* LimitSpeed negative gap :1075-1079                   */
#define PP_ST_ACC_OVERRIDE   (1u << 6)  /* some candidate hit the accT override :945-971        */
#define PP_ST_CURV_ADJUST    (1u << 7)  /* some candidate hit the curvature adjust :972-1018    */
#define PP_ST_TOO_FAR        (1u << 8)  /* "target lane too far" rule fired :1358-1369          */
#define PP_ST_BRAKE          (1u << 9)  /* a LimitSpeed returned BRAKE :1109                    */
#define PP_ST_MAXBRAKE       (1u << 10) /* a LimitSpeed returned MAXBRAKE :1101                 */
#define PP_ST_ADJUST         (1u << 11) /* a LimitSpeed returned ADJUST :1131                   */
#define PP_ST_KEEP           (1u << 12) /* a LimitSpeed returned KEEP :1146                     */
#define PP_ST_LANE_CLOSED    (1u << 13) /* some lane was closed by the planner :405-444         */
#define PP_ST_JUMP_RULE      (1u << 14) /* two-lane jump replaced by adjacent/ego lane :473-479 */

/* ---- cost modes --------------------------------------------------------------------------- */
/* PP_COST_REFERENCE: the reference's decision (planner lane, max_speed) always wins; the other
 *   candidates are ranked behind it by the comfort term. winner's next_x/next_y == reference.
 * PP_COST_COMFORT: pure comfort/lane-score cost, argmin is data dependent. */
#define PP_COST_REFERENCE 0
#define PP_COST_COMFORT   1

/* ---- scene batch (SoA; all arrays caller owned, device resident for pp_eval) ------------- */
/* Index conventions: per-scene scalars [s]; prev points [i * n_scenes + s] (i < PP_PREV_KEEP);
 * cars [j * n_scenes + s] (j < car_stride). Car ids of one scene must be ascending over j < n_cars
 * (the reference iterates a std::map<int, Car>, src/main.cpp:1194, 377, 1388). */
typedef struct pp_scene_batch {
    int64_t n_scenes;
    int32_t car_stride;            /* number of car columns (<= PP_MAX_CARS)                  */
    int32_t tab_slots;             /* car-table slots per scene (<= PP_MAX_CARS; see tab_*)    */
    const double*  ego_x;          /* telemetry x, src/main.cpp:1233                           */
    const double*  ego_y;          /* telemetry y                                              */
    const double*  ego_yaw_deg;    /* telemetry yaw (degrees)                                  */
    const double*  ego_speed_mph;  /* telemetry speed (mph), /2.237 at src/main.cpp:1239       */
    const double*  prev_x;         /* previous_path_x[0..9]                                    */
    const double*  prev_y;         /* previous_path_y[0..9]                                    */
    const int32_t* n_prev;         /* previous_path size (>=10 => first 10 used, else none)    */
    const int32_t* prev_target_lane; /* the cross-frame `target_lane` capture, src/main.cpp:1195 */
    const int32_t* n_cars;         /* sensor_fusion rows used (<= car_stride)                  */
    const int32_t* car_id;
    const double*  car_x;
    const double*  car_y;
    const double*  car_vx;
    const double*  car_vy;
    /* Optional persistent car table: the reference's cross-frame `std::map<int, Car>
     * sensor_fusion_cars` (src/main.cpp:1194, 1325-1350). NULL tab_valid = a fresh table every
     * frame. Otherwise the scene's table is tab_slots slots [k * n_scenes + s] in std::map order:
     * slot k holds car id tab_id[k] (ascending over k; tab_id NULL: slot k is id k), and every car
     * id of this frame's sensor_fusion rows is one of the slot ids (pp_plan_frame, pp_serve and the
     * rollout lay the table out over the union of the stored ids and the frame's ids; any int
     * ids). Visiting the slots in order, a reported car is re-matched and its slot overwritten, or
     * erased (valid = 0) when matching fails (:1336-1340); an unreported valid slot is the car's
     * stale entry, which the planner still uses; an invalid unreported slot is no car. */
    int32_t* tab_id;
    int32_t* tab_valid;
    int32_t* tab_lane;
    double*  tab_s;
    double*  tab_d;
    double*  tab_vs;
    double*  tab_vd;
    double*  tab_vx;
    double*  tab_vy;
} pp_scene_batch;

/* ---- parameters ---------------------------------------------------------------------------- */
typedef struct pp_params {
    int32_t n_points;      /* horizon N incl. kept previous points (reference 50)            */
    int32_t n_speeds;      /* speeds per lane: k = 0 is max_speed, k >= 1 uses speed_offsets   */
    int32_t cost_mode;     /* PP_COST_REFERENCE | PP_COST_COMFORT                             */
    int32_t emit_paths;    /* 1: write every candidate's path to pp_result.paths              */
    double  speed_offsets[PP_MAX_SPEEDS]; /* v_k = clamp(ego_speed + speed_offsets[k-1], 0, max_speed) */
    /* tunables, src/main.cpp:39-49 (defaults = reference values) */
    double  relaxed_acc;                    /* 5    */
    double  min_relaxed_acc_while_braking;  /* 4    */
    double  maximum_acc;                    /* 8    */
    double  max_speed;                      /* 22.2 */
    double  car_length;                     /* 4.5  */
    double  safety_distance;                /* 2    */
    double  keep_distance;                  /* 10   */
    double  keep_distance_leeway;           /* 0.5  */
    /* Monte-Carlo sensor noise (BASELINE config 4). n_draws = D > 1
     * evaluates every scene D times: draw 0 is the scene as given, draw d >= 1 perturbs every
     * sensor_fusion car j by (sigma_pos g0, sigma_pos g1, sigma_vel g2, sigma_vel g3) added to
     * (x, y, vx, vy), g = pp_mc_gauss(noise_seed, noise_first_scene + s, d, j, q). Candidates per
     * scene become C = D * 3 * n_speeds, c = (d * 3 + lane) * n_speeds + k. The per-scene decision
     * averages each (lane, k) cost over the draws (summed in draw order, then / D) and takes the
     * first minimum; next_x/next_y are the draw-0 (nominal) trajectory of that (lane, k), winner
     * = lane * n_speeds + k. emit_paths must be 0 when D > 1. */
    int32_t n_draws;                        /* 0 or 1: off                                  */
    int32_t _pad_mc;
    uint64_t noise_seed;
    int64_t noise_first_scene;              /* global index of the batch's scene 0 (shards)  */
    double  noise_pos_sigma;                /* 0.5 m                        */
    double  noise_vel_sigma;                /* 0.5 m/s                                       */
} pp_params;

/* ---- optional per-scene diagnostics (the planner's intermediate state) --------------------- */
typedef struct pp_scene_info {
    double  ego_x, ego_y, ego_speed, ego_acc;      /* after the derivation, src/main.cpp:1261-1320 */
    double  ego_s, ego_d, ego_vs, ego_vd;
    double  ref_ratio[PP_NUM_LANES];               /* Map::reference_waypoint_ratio          */
    double  lane_score[PP_NUM_LANES];              /* LaneChangePlanner scores :450-471       */
    int32_t ref_wp;                                /* Map::reference_waypoint_id             */
    int32_t ego_lane;
    int32_t target_lane;                           /* after planner + too-far rule           */
    int32_t lane_open_mask;
    int32_t n_matched_cars;
    int32_t in_lane_car;                           /* follow car id or -1, :1383-1400         */
    int32_t _pad[2];
} pp_scene_info;

/* ---- results (caller owned; device resident for pp_eval) ---------------------------------- */
/* C = PP_NUM_LANES * n_speeds (times n_draws for Monte-Carlo), candidate c = lane * n_speeds + k.
 * next_x/next_y: point-major like the batch's prev_x/prev_y, [i * n_scenes + s] (i < n_points;
 * points i >= n_out[s] are 0); cost: [s * C + c];
 * paths (emit_paths): [((s * n_points + i) * C + c) * 2 + {0:x, 1:y}], path_len: [s * C + c]. */
typedef struct pp_result {
    int32_t*  winner;
    int32_t*  n_out;          /* points written to next_x/next_y for the scene (<= n_points)  */
    double*   next_x;
    double*   next_y;
    double*   cost;
    uint32_t* status;
    double*   paths;          /* optional (emit_paths)                                          */
    int32_t*  path_len;       /* optional (emit_paths)                                          */
    pp_scene_info* info;      /* optional                                                       */
    double*   draw_mean_cost; /* optional (n_draws > 1): [s * 3 * n_speeds + lane * n_speeds + k],
                                 the draw-averaged cost the decision minimises                  */
} pp_result;

/* ---- API ----------------------------------------------------------------------------------- */
typedef struct pp_map pp_map;

void    pp_params_default(pp_params* p);
int32_t pp_num_candidates(const pp_params* p);
int32_t pp_num_lanes(void);           /* PP_NUM_LANES of this build */
int32_t pp_max_cars(void);            /* PP_MAX_CARS of this build */

/* Map::Init (src/main.cpp:89-131) on the host (bit-identical to the reference's); the lane
 * geometry is uploaded lazily per device. n >= 3 waypoints, any size. */
int32_t pp_map_create(const double* wx, const double* wy, int32_t n, pp_map** out);
/* Map::Init on `device` from DEVICE waypoint arrays: the same formulas
 * with the device's atan2/cos (the reference's lane centres within ~1e-12 m instead of bit for
 * bit); tables mirrored to the host. Maps of any size (> 600 waypoints: the planner reads the map
 * from global memory instead of staging it in LDS). Synchronous on hip_stream. */
int32_t pp_map_create_device(const double* d_wx, const double* d_wy, int32_t n, int32_t device, void* hip_stream,
                             pp_map** out);
int32_t pp_map_destroy(pp_map* m);
/* host copy of the derived geometry: per waypoint {ref.x, ref.y, nx, ny, lc0.x, lc0.y, lc1.x,
 * lc1.y, ...} (4 + 2 * PP_NUM_LANES doubles) — the Map::Init known-answer output. */
int32_t pp_map_geometry(const pp_map* m, double* out, int32_t n);

/* Pre-size the per-device workspace (optional; pp_eval grows it on demand, which allocates). */
int32_t pp_reserve(pp_map* m, int32_t device, int64_t max_scenes);

/* Evaluate a batch. All batch/result pointers are device memory on `device`; `hip_stream` is a
 * hipStream_t (NULL = default stream). Asynchronous w.r.t. the host. Thread-safe: every stream
 * has its own device workspace, so calls on different streams may overlap; calls on one stream
 * run in its order. */
int32_t pp_eval(pp_map* m, const pp_scene_batch* in, const pp_params* prm, pp_result* out,
                int32_t device, void* hip_stream);

/* One telemetry frame, host memory in/out: the onMessage replacement (C = 1, reference decision).
 * prev_x/prev_y hold n_prev points (only the first 10 are read when n_prev >= 10); the car arrays
 * hold n_cars rows (<= PP_MAX_CARS) in any order with any int ids (sorted by id internally, the
 * last row of a repeated id wins, as std::map assignment does). The car table persists across
 * calls like the reference's (see pp_plan_reset); PP_ERR_ARG if the table would hold more than
 * PP_MAX_CARS distinct cars. *target_lane is read (cross-frame state) and updated. Writes up to
 * 50 points. Calls on one map and device are serialised. */
int32_t pp_plan_frame(pp_map* m, int32_t device,
                      double ego_x, double ego_y, double ego_yaw_deg, double ego_speed_mph,
                      const double* prev_x, const double* prev_y, int32_t n_prev,
                      const int32_t* car_id, const double* car_x, const double* car_y,
                      const double* car_vx, const double* car_vy, int32_t n_cars,
                      int32_t* target_lane, double* next_x, double* next_y, int32_t* n_out);

/* Deterministic synthetic scenes (Philox4x32-10 keyed by seed, counter = global scene index),
 * generated on `device` into caller-owned device buffers described by `out` (car_stride = 12).
 * first_scene = global index of out's scene 0 (for multi-GPU shards). */
int32_t pp_synth_scenes(pp_map* m, uint64_t seed, int64_t first_scene, pp_scene_batch* out,
                        int32_t device, void* hip_stream);
/* The same generator on the host (identical bits except ego_yaw_deg, which goes through atan2). */
int32_t pp_synth_scenes_host(const pp_map* m, uint64_t seed, int64_t first_scene,
                             pp_scene_batch* out);

/* ---- closed-loop rollout ------------------------------------------- */
/* A simulator shim closes the loop around the planner: per frame, pp_eval plans every scene, then
 * the simulator drives `consume` points of each plan (the ego ends on point consume-1; speed and
 * yaw from the last two driven points; previous_path = the undriven rest), sets the cross-frame
 * target lane (src/main.cpp:1195) to the plan's lane (winner / n_speeds), advances the traffic by
 * consume * 0.02 s and reports the cars within sensor_range (ascending id) as the next frame's
 * sensor_fusion; the others become stale car-table entries (tab_* above, required). */
typedef struct pp_traffic {        /* device SoA [j * n_scenes + s]; car j has id j, table slot j  */
    int32_t  n_cars;               /* cars per scene (<= PP_MAX_CARS)                               */
    int32_t  _pad;
    int32_t* lane;                 /* lane-centre polyline it follows                              */
    int32_t* seg;                  /* segment (ends at waypoint seg) and fraction t on it          */
    double*  t;
    double*  offset;               /* lateral offset from the lane centre (right-hand normal)      */
    double*  speed;                /* m/s along the lane                                           */
} pp_traffic;

typedef struct pp_rollout_cfg {
    int32_t n_frames;
    int32_t consume;               /* points the simulator drives per frame (>= 1)                 */
    double  sensor_range;          /* metres; cars farther from the ego are not reported           */
} pp_rollout_cfg;

/* Optional per-frame records, [f * n_scenes + s] (plans: [(f * n_points + i) * n_scenes + s]);
 * any pointer may be NULL. The ego fields are the telemetry the frame was planned from. */
typedef struct pp_rollout_log {
    double*   ego_x;
    double*   ego_y;
    double*   ego_speed_mph;
    int32_t*  target_lane;        /* after the frame (the plan's lane)                             */
    int32_t*  winner;
    int32_t*  n_out;
    uint32_t* status;
    int32_t*  n_cars;             /* sensor_fusion rows the frame was planned from                 */
    double*   plan_x;
    double*   plan_y;
} pp_rollout_log;

/* Runs cfg->n_frames frames; `telemetry` (with its car table: tab_slots >= traffic n_cars, slot j
 * = car j, tab_id NULL or j), `traffic` and `result` (per-frame plan buffers, pp_eval layout) are
 * device state updated in place, so consecutive calls continue the episode. n_draws must be <= 1
 * and emit_paths 0. */
int32_t pp_rollout(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                   const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                   pp_rollout_log* log, int32_t device, void* hip_stream);

/* ---- rollout judge: incidents of a closed-loop drive ---------------------------------------- */
/* The simulator this planner was written for counts the distance driven without an incident: a
 * collision, more than 50 mph, total acceleration over 10 m/s^2, jerk over 10 m/s^3, or too long
 * outside a lane. The simulator is not part of the reference, so the definitions here are THIS
 * LIBRARY'S OWN, modelled on those published rules (DESIGN.md "Rollout judge" states them in
 * full); nothing is or can be compared with the simulator. The judge looks at every driven step
 * (0.02 s) of a frame: the ego's plan points against the limits, the lane-centre polylines and
 * the rectangles of all traffic cars, whatever the sensor range. */
#define PP_JUDGE_RING     64          /* velocity ring entries per scene (a power of two)          */
#define PP_INC_KINDS      5           /* incident kinds: the bit numbers below                     */
#define PP_INC_COLLISION  (1u << 0)   /* ego and car rectangles overlap (separating-axis sep <= 0) */
#define PP_INC_SPEED      (1u << 1)   /* step speed > speed_limit_mph                              */
#define PP_INC_ACC        (1u << 2)   /* |windowed acceleration| > max_acc                         */
#define PP_INC_JERK       (1u << 3)   /* |windowed jerk| > max_jerk                                */
#define PP_INC_OFF_LANE   (1u << 4)   /* more than off_lane_steps consecutive steps off every lane */

typedef struct pp_judge_cfg {
    double  speed_limit_mph;       /* 50                                                           */
    double  max_acc;               /* 10 m/s^2                                                     */
    double  max_jerk;              /* 10 m/s^3                                                     */
    double  ego_length;            /* 4.5 m, along the heading                                     */
    double  ego_width;             /* 2.0 m                                                        */
    double  car_length;            /* 4.5 m, along the car's lane tangent                          */
    double  car_width;             /* 2.0 m                                                        */
    double  lane_tol;              /* 1.0 m: farther than this from every lane centre is off-lane  */
    int32_t acc_window;            /* 10 steps: a_n = (v_n - v_{n-Wa}) / (Wa 0.02)                 */
    int32_t jerk_window;           /* 50 steps: j_n = (a_n - a_{n-Wj}) / (Wj 0.02)                 */
    int32_t off_lane_steps;        /* 150: the off-lane run may last this many steps               */
    int32_t _pad;
} pp_judge_cfg;                    /* 1 <= acc_window, 1 <= jerk_window, their sum <= 63           */

/* Judge state of a batch (SoA, caller owned; device resident for pp_judge_frame and
 * pp_rollout_judged, host memory for pp_judge_frame_host), S = the telemetry's n_scenes. Index
 * conventions: per-scene scalars [s]; per-kind records [kind * S + s] (kind < PP_INC_KINDS, the bit
 * number of PP_INC_*); ring entries [k * S + s] (k < PP_JUDGE_RING; the velocity of the episode's
 * step n, 1-based, is entry n & (PP_JUDGE_RING - 1)). A scene whose steps[s] is 0 on entry starts
 * a fresh episode: every other field of it is initialised by the call, so a zero-filled state is a
 * valid start and a state is reused by zeroing `steps` alone. */
typedef struct pp_judge {
    int32_t*  steps;               /* driven steps judged so far (carried; 0 = fresh episode)      */
    uint32_t* flags;               /* OR of PP_INC_* seen so far                                   */
    int32_t*  count;               /* [kind * S + s] steps in violation                            */
    int32_t*  first_step;          /* [kind * S + s] episode step of the first violation, 0: none  */
    int32_t*  first_car;           /* traffic car of the first collision + 1, 0: none              */
    int32_t*  seg_hint;            /* carried: lane-centre segment nearest to the ego              */
    int32_t*  off_run;             /* carried: current run of consecutive off-lane steps           */
    double*   head_x;              /* carried: unit heading of the last step that moved            */
    double*   head_y;
    double*   ring_vx;             /* carried: [k * S + s] step velocities (m/s)                   */
    double*   ring_vy;
    double*   dist;                /* metres driven                                                */
    double*   clean_dist;          /* dist at the end of the last step before the first incident   */
    double*   min_sep;             /* smallest separation to any car so far (+inf: none judged)    */
    double*   max_speed_mph;       /* running maxima of the judged quantities                      */
    double*   max_acc;
    double*   max_jerk;
} pp_judge;

void    pp_judge_cfg_default(pp_judge_cfg* c);
/* Judges the `consume` driven steps of ONE frame from the pre-frame state: `telemetry` (ego_x,
 * ego_y, ego_yaw_deg are read) and `traffic` as they are before the simulator moves them, `plan`
 * (n_out, next_x, next_y) as pp_eval wrote it. For callers that run their own loop around pp_eval:
 * call it after pp_eval and before moving the ego and the traffic. Nothing but `state` is written.
 * The traffic is trusted as pp_rollout trusts it: every car's lane < PP_NUM_LANES and 0 <= seg <
 * the map's waypoint count are the caller's duty (they index the lane tables unchecked), and
 * n_out[s] must not exceed the points next_x/next_y hold. Device pointers; asynchronous on
 * hip_stream. */
int32_t pp_judge_frame(pp_map* m, const pp_scene_batch* telemetry, const pp_traffic* traffic,
                       const pp_result* plan, int32_t consume, const pp_judge_cfg* cfg, pp_judge* state,
                       int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_judge_frame_host(const pp_map* m, const pp_scene_batch* telemetry, const pp_traffic* traffic,
                            const pp_result* plan, int32_t consume, const pp_judge_cfg* cfg, pp_judge* state);
/* pp_rollout with the judge: per frame pp_eval, the judge, then the simulator, on the one stream.
 * Everything pp_rollout writes is written exactly as pp_rollout writes it. */
int32_t pp_rollout_judged(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                          const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                          pp_rollout_log* log, int32_t device, void* hip_stream,
                          const pp_judge_cfg* jcfg, pp_judge* state);

/* ---- reactive traffic: every car follows the vehicle ahead of it in its lane ------------------- */
/* pp_rollout's traffic keeps its speed for ever and drives through the ego and through other cars.
 * Here each car follows the nearest vehicle ahead of it in its lane (another car, or the ego where
 * it stands within lateral_reach of that lane's centre) by the Intelligent Driver Model. One call
 * updates traffic.speed in place for one frame of `consume` steps (dt = consume 0.02 s) from the
 * PRE-FRAME state; positions are not touched (the simulator moves the cars). The definitions are
 * THIS LIBRARY'S OWN (DESIGN.md "Reactive traffic" states them in full); the reference has no
 * simulator and nothing is compared with it. In short, with v a car's speed, v0 its desired speed,
 * vl its leader's speed and g the net gap along the lane (centre gap minus the half lengths):
 *   free = 1 - (v / v0)^4
 *   s*   = min_gap + max(0, v time_headway + v (v - vl) / (2 sqrt(max_acc comfort_brake)))
 *   a    = max_acc (free - (s* / max(g, gap_floor))^2), or max_acc free with no leader within horizon
 *   v'   = min(max(v + max(a, -max_brake) dt, 0), v0)
 * Every v' comes from the pre-frame speeds of all cars. A car with v0 <= 0 (parked) is left alone. */
typedef struct pp_follow_cfg {
    double  max_acc;               /* 2.0 m/s^2: the acceleration on a free road from rest         */
    double  comfort_brake;         /* 3.0 m/s^2: the deceleration the model approaches a leader by */
    double  max_brake;             /* 8.0 m/s^2: a is never below -max_brake                       */
    double  time_headway;          /* 1.2 s                                                        */
    double  min_gap;               /* 2.0 m: the net gap kept at standstill                        */
    double  gap_floor;             /* 0.5 m: net gaps below this (overlapping cars) count as this  */
    double  horizon;               /* 150 m: a vehicle with a net gap beyond this is no leader     */
    double  car_length;            /* 4.5 m                                                        */
    double  ego_length;            /* 4.5 m                                                        */
    double  lateral_reach;         /* 2.0 m: the ego occupies a lane whose centre is this near     */
    int32_t react_to_ego;          /* 1: the ego is a leader candidate; 0: the cars do not see it  */
    int32_t _pad;
} pp_follow_cfg;                   /* max_acc, comfort_brake, max_brake, gap_floor > 0; horizon,
                                      lengths and lateral_reach >= 0                               */

/* Follow state of a batch (SoA, caller owned; device resident for pp_traffic_follow and
 * pp_rollout_reactive, host memory for pp_traffic_follow_host), S = the telemetry's n_scenes, per-car
 * arrays [j * S + s] for j < traffic.n_cars. A scene whose started[s] is 0 on entry starts a fresh
 * episode: its cars' desired speeds are captured from traffic.speed and every other field of it is
 * written by the call, so a zero-filled state is a valid start and a state is reused by zeroing
 * `started` alone. */
typedef struct pp_follow {
    int32_t* started;              /* 0 = fresh episode; set to 1 by the call                      */
    int32_t* ego_seg;              /* carried: lane-centre segment nearest to the ego + 1, 0: none */
    double*  desired;              /* [j * S + s] v0, captured on the fresh call                   */
    double*  next_speed;           /* [j * S + s] staging (the new speeds before they are written) */
    int32_t* leader;               /* [j * S + s] record: -1 none, n_cars the ego, else the car    */
    double*  gap;                  /* [j * S + s] record: the net gap g, +inf with no leader       */
} pp_follow;

void    pp_follow_cfg_default(pp_follow_cfg* c);
/* Updates traffic->speed for ONE frame from the pre-frame state: `telemetry` (ego_x, ego_y,
 * ego_speed_mph are read) and `traffic` (lane, seg, t, speed) as they are before the simulator
 * moves them. For callers that run their own loop around pp_eval: call it before pp_judge_frame and
 * before moving the traffic, so that the judge and the move use the speeds of this frame. Writes
 * traffic->speed and `state` only. lane and seg are trusted as pp_rollout trusts them. Device
 * pointers; asynchronous on hip_stream. */
int32_t pp_traffic_follow(pp_map* m, const pp_scene_batch* telemetry, pp_traffic* traffic, int32_t consume,
                          const pp_follow_cfg* cfg, pp_follow* state, int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_traffic_follow_host(const pp_map* m, const pp_scene_batch* telemetry, pp_traffic* traffic,
                               int32_t consume, const pp_follow_cfg* cfg, pp_follow* state);
/* pp_rollout with reactive traffic: per frame pp_eval, the follow update, the judge (only when
 * jstate is not NULL; jcfg is then required), then the simulator, on the one stream. The judge
 * advances the cars over the frame's steps by the speeds the simulator then moves them by, and the
 * simulator reports those speeds in the next telemetry. */
int32_t pp_rollout_reactive(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                            const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                            pp_rollout_log* log, int32_t device, void* hip_stream,
                            const pp_judge_cfg* jcfg, pp_judge* jstate,
                            const pp_follow_cfg* fcfg, pp_follow* fstate);

/* ---- lane-changing traffic: a car moves to a neighbour lane when MOBIL says so ----------------- */
/* Reactive traffic never leaves its lane: a faster car queues behind a slower one for ever and no car
 * ever moves into the ego's lane. Here the cars change lanes by MOBIL ("minimising overall braking
 * induced by lane changes") on the accelerations of the model above. One call runs AFTER
 * pp_traffic_follow of the same frame and reads that call's records (desired, leader, gap, ego_seg)
 * and the speeds it wrote. THIS LIBRARY'S OWN definitions (DESIGN.md "Lane-changing traffic" states
 * them in full). In short, per call and scene: every car's offset returns to its home value at
 * lateral_speed and its wait runs down; a car that is not parked, not waiting and not in transit
 * (offset == home) is a candidate for lane - 1 and lane + 1; on the target lane it would get the new
 * leader n and the new follower f (other cars of that lane, and the ego where it occupies it), and
 * leave its old follower o behind. With a the IDM acceleration before and a' after the change:
 *   safe    = net gaps to n and f >= min_gap, a_f' >= -safe_brake, a_j' >= -safe_brake
 *   gain    = (a_j' - a_j) + politeness ((a_f' - a_f) + (a_o' - a_o))     (the ego never gains)
 *   surplus = gain - threshold -/+ right_bias
 * and the ONE candidate of the scene with the largest surplus > 0 is placed on its new lane at the
 * nearest point of that lane's centre, with the offset that keeps it where it is; it then waits
 * min_interval_steps. A car in transit counts only in its new lane. */
typedef struct pp_lane_change_cfg {
    double  politeness;            /* 0.3: weight of the other drivers' gain                       */
    double  threshold;             /* 0.2 m/s^2: the gain a change must exceed (+inf: never change) */
    double  right_bias;            /* 0.0 m/s^2: added to the threshold of a change to lane - 1,
                                      subtracted from that of a change to lane + 1                 */
    double  safe_brake;            /* 3.0 m/s^2: no change makes anyone brake harder than this     */
    double  lateral_speed;         /* 1.5 m/s: how fast the offset returns to its home value       */
    double  ego_desired_speed;     /* 22.2 m/s: v0 of the ego where it would become the new follower */
    int32_t min_interval_steps;    /* 250: driven steps a car waits after beginning a change       */
    int32_t _pad;
} pp_lane_change_cfg;              /* politeness >= 0; safe_brake, lateral_speed, ego_desired_speed
                                      > 0; min_interval_steps >= 0; no NaN                         */

/* Lane-change state of a batch (SoA, caller owned; device resident for pp_traffic_lane_change and
 * pp_rollout_lane_changing, host memory for pp_traffic_lane_change_host), S = the telemetry's
 * n_scenes, per-car arrays [j * S + s] for j < traffic.n_cars. A scene whose started[s] is 0 on
 * entry starts a fresh episode: its cars' home offsets are captured from traffic.offset and every
 * other field of it is written by the call, so a zero-filled state is a valid start and a state is
 * reused by zeroing `started` alone. */
typedef struct pp_lane_change {
    int32_t* started;              /* 0 = fresh episode; set to 1 by the call                      */
    int32_t* n_changes;            /* changes begun in this scene so far                           */
    int32_t* last_car;             /* car + 1 that began a change in the LAST call, 0: none        */
    int32_t* last_dir;             /* -1 / +1 of that change, 0: none                              */
    double*  home;                 /* [j * S + s] the offset the car returns to (captured fresh)   */
    int32_t* wait;                 /* [j * S + s] driven steps until the car may change again      */
    int32_t* changes;              /* [j * S + s] changes this car has begun                       */
    double*  arc;                  /* [j * S + s] staging: the car's arc on its own lane           */
    double*  gain;                 /* [j * S + s] record: best surplus of this call, -inf: not eligible */
    int32_t* dir;                  /* [j * S + s] record: direction of that surplus, 0: none       */
} pp_lane_change;

void    pp_lane_change_cfg_default(pp_lane_change_cfg* c);
/* Lets the traffic change lanes for ONE frame. Call it after pp_traffic_follow of the same frame
 * (same telemetry, traffic, consume, fcfg and fstate) and before pp_judge_frame and before moving
 * the traffic. Writes traffic->lane, seg, t, offset and `state`; never traffic->speed or `fstate`. A
 * scene whose fstate->started is 0 is left alone; with no cars nothing is touched. PP_ERR_ARG (before
 * any HIP call) for a NULL argument or state array, a follow cfg or state pp_traffic_follow would
 * refuse, a cfg outside the ranges above, or consume < 1. Device pointers; asynchronous on
 * hip_stream. */
int32_t pp_traffic_lane_change(pp_map* m, const pp_scene_batch* telemetry, pp_traffic* traffic, int32_t consume,
                               const pp_follow_cfg* fcfg, const pp_follow* fstate,
                               const pp_lane_change_cfg* cfg, pp_lane_change* state,
                               int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_traffic_lane_change_host(const pp_map* m, const pp_scene_batch* telemetry, pp_traffic* traffic,
                                    int32_t consume, const pp_follow_cfg* fcfg, const pp_follow* fstate,
                                    const pp_lane_change_cfg* cfg, pp_lane_change* state);
/* pp_rollout_reactive with lane changes: per frame pp_eval, the follow update, the lane changes, the
 * judge (only when jstate is not NULL), then the simulator, on the one stream. lcfg and lstate both
 * NULL: exactly pp_rollout_reactive. */
int32_t pp_rollout_lane_changing(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                                 const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                                 pp_rollout_log* log, int32_t device, void* hip_stream,
                                 const pp_judge_cfg* jcfg, pp_judge* jstate,
                                 const pp_follow_cfg* fcfg, pp_follow* fstate,
                                 const pp_lane_change_cfg* lcfg, pp_lane_change* lstate);

/* Rollout start state: writes the synthetic scenes of pp_synth_scenes (same seed and indices)
 * into `telemetry` and their traffic into `out` (n_cars = 12): car j starts exactly where the
 * scene reports it, on its lane with its lateral offset and speed. Empties the car table of
 * `telemetry` when its tab_valid is set. */
int32_t pp_synth_traffic(pp_map* m, uint64_t seed, int64_t first_scene, pp_scene_batch* telemetry,
                         pp_traffic* out, int32_t device, void* hip_stream);
int32_t pp_synth_traffic_host(const pp_map* m, uint64_t seed, int64_t first_scene,
                              pp_scene_batch* telemetry, pp_traffic* out);

/* ---- episode starts: start states made to be driven and judged ------------------------------- */
/* pp_synth_traffic's scenes are the benchmark's snapshot: the previous path ends at the ego, the judge
 * starts from v_0 = 0 and the cars are dropped with no regard to each other or to the ego, so the
 * judge of a drive from them reports on the generator. pp_synth_episode writes a start that can be
 * driven: the ego on a lane centre at speed ve along the segment's tangent u, its previous path the
 * ten points p + (k + 1) ve 0.02 u AHEAD of it (n_prev = 0 at rest); n_cars cars placed one after the
 * other, each on a random lane ahead of (probability ahead_share) or behind everything placed on that
 * lane so far, the ego counting as present on every lane, at the net gap the car-following rule asks
 * for, s*(follower, leader) of `gap_rule` (pp_follow_cfg above), plus gap_slack plus U[0, extra_gap);
 * all of them reported in the frame-0 telemetry (ids 0..n_cars-1), the car table emptied. THIS
 * LIBRARY'S OWN definitions (DESIGN.md "Episode starts" states them in full). A scene depends only
 * on (seed, first_scene + s, cfg, gap_rule): shards concatenate; the stream is not pp_synth_scenes'.
 *
 * `jstate` (optional) becomes a WARM judge state: steps = PP_JUDGE_RING, every ring entry the start
 * velocity ve u, head = u, seg_hint = the ego's segment, min_sep = +inf, every record 0. The judge
 * takes it for a carried state, so a start at speed records no start transient. EPISODE STEP NUMBERS
 * ARE THEREFORE OFFSET BY PP_JUDGE_RING: after F frames steps = PP_JUDGE_RING + F consume, and a
 * first_step f is driven step f - PP_JUDGE_RING. `fstate` (optional) is reset for a fresh episode
 * (started = 0, ego_seg = 0). */
typedef struct pp_episode_cfg {
    int32_t n_cars;          /* 12; 0 <= n_cars <= min(PP_MAX_CARS, car_stride, tab_slots)          */
    int32_t _pad;
    double  ego_speed_min;   /* 0 m/s                                                              */
    double  ego_speed_max;   /* 20 m/s; both 0: every ego starts at rest                           */
    double  car_speed_min;   /* 5 m/s                                                              */
    double  car_speed_max;   /* 25 m/s                                                             */
    double  ahead_share;     /* 0.75: probability that a car is placed ahead of the ego            */
    double  extra_gap;       /* 40 m: U[0, extra_gap) on top of the required net gap               */
    double  offset_jitter;   /* 0.3 m: lateral offset U(-j, j)                                     */
    double  gap_slack;       /* 1e-6 m added to every required gap (covers the arcs' rounding)     */
} pp_episode_cfg;            /* every field >= 0, min <= max, ahead_share <= 1                      */

void    pp_episode_cfg_default(pp_episode_cfg* c);
/* Device pointers; asynchronous on hip_stream. traffic's arrays hold at least cfg->n_cars cars;
 * traffic->n_cars is set. gap_rule NULL: pp_follow_cfg_default. PP_ERR_ARG (before any HIP call) for
 * a NULL, n_cars out of range, a bad cfg, a gap_rule pp_traffic_follow would refuse (or whose
 * time_headway or min_gap is negative or NaN), or a ring too
 * short for the traffic: (n_cars + 1) (s*(vmax, vmin) + gap_slack + extra_gap + max length) above the
 * shortest lane's loop, vmax the larger speed maximum and vmin the smaller minimum (the defaults
 * allow 33 cars on the highway map; denser traffic needs narrower speed ranges). */
int32_t pp_synth_episode(pp_map* m, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                         const pp_follow_cfg* gap_rule, pp_scene_batch* telemetry, pp_traffic* traffic,
                         pp_judge* jstate, pp_follow* fstate, int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_synth_episode_host(const pp_map* m, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                              const pp_follow_cfg* gap_rule, pp_scene_batch* telemetry, pp_traffic* traffic,
                              pp_judge* jstate, pp_follow* fstate);

/* ---- judge summary: a judged batch as figures per group of scenes ------------------------------ */
/* A judged drive ends as per-scene arrays (pp_judge). pp_judge_summary reduces them on the device to
 * one row of figures per GROUP of scenes: groups are contiguous, scene s belongs to group
 * g = s / scenes_per_group, G = ceil(S / scenes_per_group), the last group may be short (a sweep lays
 * its sets out this way, shards concatenate this way, scenes_per_group = S gives one row). THIS
 * LIBRARY'S OWN definitions (DESIGN.md "Judge summary and parameter sweeps" states them in full).
 * A scene with steps[s] == 0 is UNJUDGED: a fresh state defines nothing else of it, so it counts in
 * n_scenes and n_unjudged only. A judged scene whose dist or clean_dist is NaN or infinite counts in
 * n_nonfinite and is left out of the four dist figures and the histogram, nothing else.
 * The histogram of clean_dist: inv_w = hist_bins / hist_max (one host division), q = clean_dist inv_w,
 * bin = q >= hist_bins - 1 ? hist_bins - 1 : (int)q (a negative clean_dist, which the judge never
 * produces, counts in bin 0).
 * The two sums are ONE FIXED EXPRESSION, the same bits on host and device and from run to run: with
 * the group's values x_0.. in scene order (a scene left out counts +0.0), tile t = x[256 t .. 256 t +
 * 255] padded with +0.0, tree256(v): for w = 128, 64, .., 1: v[i] += v[i + w] for i < w, result v[0];
 * T_t = tree256(tile t); u_i = the sum from +0.0, in ascending t, of T_t over t = i (mod 256); the
 * group's sum = tree256(u). Tiles start at the group's first scene: a row depends on its own group's
 * scenes only. */
#define PP_STATS_MAX_BINS 1024
typedef struct pp_summary_cfg {
    int64_t scenes_per_group;      /* E >= 1                                                        */
    int32_t hist_bins;             /* B, 1..PP_STATS_MAX_BINS                                       */
    int32_t _pad;
    double  hist_max;              /* metres, finite, > 0: the clean_dist histogram covers [0, hist_max),
                                      the last bin also holds everything beyond                     */
    int64_t out_first;             /* row of group 0 in the stats arrays                            */
    int64_t out_stride;            /* rows the stats arrays hold (0: G, and then out_first must be 0) */
} pp_summary_cfg;

/* Caller owned (device memory for pp_judge_summary and pp_rollout_sweep, host memory for
 * pp_judge_summary_host); R = out_stride rows; per row [r], per kind [kind * R + r] (kind <
 * PP_INC_KINDS), histogram [b * R + r] (b < hist_bins). */
typedef struct pp_judge_stats {
    int64_t* n_scenes;             /* scenes of the group                                          */
    int64_t* n_unjudged;           /* steps[s] == 0; left out of everything below                  */
    int64_t* n_nonfinite;          /* judged scenes whose dist or clean_dist is NaN or infinite    */
    int64_t* n_clean;              /* judged scenes with flags == 0                                */
    int64_t* steps;                /* sum of steps                                                 */
    int64_t* scenes_with;          /* [kind * R + r] scenes with count[kind] > 0                   */
    int64_t* steps_in;             /* [kind * R + r] sum of count[kind]                            */
    int32_t* first_step_min;       /* [kind * R + r] smallest first_step > 0, 0: none              */
    double*  dist_sum;             /* the two sums (the expression above)                          */
    double*  clean_dist_sum;
    double*  clean_dist_min;       /* +inf / -inf where the group has no finite judged scene       */
    double*  clean_dist_max;
    double*  min_sep;              /* min over judged scenes, NaN ignored (+inf stays +inf)        */
    double*  max_speed_mph;        /* max over judged scenes, NaN ignored, -inf: none              */
    double*  max_acc;
    double*  max_jerk;
    int64_t* hist;                 /* [b * R + r] scenes with a finite clean_dist in bin b         */
} pp_judge_stats;

/* Rows out_first .. out_first + G - 1 of `stats` are OVERWRITTEN, nothing else is written, `state` (S =
 * n_scenes scenes) is only read. Device pointers; asynchronous on hip_stream, no host synchronisation
 * (the tile partials live in the stream's workspace of `m`, which grows as pp_eval's does: calls on
 * one stream are ordered by it, a call with more tiles than any before waits for the stream once).
 * PP_ERR_ARG (before any HIP call) for a NULL map, state or stats array, scenes_per_group < 1,
 * hist_bins outside 1..PP_STATS_MAX_BINS, hist_max not finite or not > 0, out_first < 0, out_stride
 * neither 0 nor >= out_first + G, out_stride 0 with out_first != 0, n_scenes < 0 or a bad device;
 * n_scenes == 0: PP_OK, nothing written. */
int32_t pp_judge_summary(pp_map* m, const pp_judge* state, int64_t n_scenes, const pp_summary_cfg* cfg,
                         pp_judge_stats* stats, int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same figures, bit for bit). */
int32_t pp_judge_summary_host(const pp_judge* state, int64_t n_scenes, const pp_summary_cfg* cfg,
                              pp_judge_stats* stats);

/* ---- parameter sweeps: the same seeded episodes driven once per parameter set ------------------- */
typedef struct pp_sweep_cfg {
    int32_t  n_sets;               /* >= 1                                                          */
    int32_t  _pad;
    uint64_t seed;                 /* pp_synth_episode's seed and first scene: every set's starts   */
    int64_t  first_scene;
    pp_rollout_cfg rollout;
    pp_summary_cfg summary;        /* out_first / out_stride are set by the sweep (ignored here):
                                      set p's group g is row p * G + g of n_sets * G rows          */
} pp_sweep_cfg;
/* Per set p, in order, on the one stream and with no host synchronisation: pp_synth_episode(seed,
 * first_scene, ecfg, fcfg as the gap rule, telemetry, traffic, jstate, fstate); lstate->started
 * zeroed (where there is an lstate); pp_rollout_lane_changing of rollout.n_frames frames with
 * sets[p] (no log); pp_judge_summary into rows p * G ... Set p's rows are, bit for bit, what those
 * calls made by hand produce. `sets` is host memory; every other buffer is the caller's device state,
 * sized for telemetry->n_scenes scenes, and `result` for the largest n_points and candidate count
 * among the sets: THE CALLER'S DUTY. lcfg and lstate both NULL: no lane changes. PP_ERR_ARG before
 * anything is launched for n_sets < 1, a NULL argument, or any set, configuration or state one of
 * those calls would refuse. */
int32_t pp_rollout_sweep(pp_map* m, const pp_params* sets, const pp_sweep_cfg* cfg,
                         const pp_episode_cfg* ecfg, const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg,
                         const pp_lane_change_cfg* lcfg, pp_scene_batch* telemetry, pp_traffic* traffic,
                         pp_result* result, pp_judge* jstate, pp_follow* fstate, pp_lane_change* lstate,
                         pp_judge_stats* stats, int32_t device, void* hip_stream);

/* ---- sensor model: what the planner is told about the traffic ---------------------------------- */
/* The simulator reports every car within sensor_range at its exact position and velocity. The sensor
 * model stands between that TRUTH and the planner: a car may be hidden behind a nearer car, a report
 * may be lost, and what is reported carries noise. THIS LIBRARY'S OWN definitions (DESIGN.md "Sensor
 * model" states them in full). The truth is `telemetry`'s ego_x, ego_y, n_cars and car rows, which
 * are only read; the sensed rows go to the state's own arrays, compacted in truth order. Per truth
 * row r (car id j, centre c), with a = c - ego, f = frame[s] before the call, gs = first_scene + s:
 *   occluded  (occlusion_radius > 0) some truth row k != r with b = c_k - ego has b.b < a.a and
 *             |b - u a|^2 <= occlusion_radius^2, u = (a.b) / (a.a) clamped to [0, 1]. Every truth row
 *             can occlude, whatever its own fate; O(rows^2) per scene
 *   dropped   (not occluded) (double)w 2^-32 < dropout_prob, w = pp_sensor_word(seed, gs, f, j)
 *   reported  x + sp g0, y + sp g1, vx + vel_sigma g2, vy + vel_sigma g3 with sp = pos_sigma +
 *             pos_sigma_per_m sqrt(a.a) and g_q = pp_sensor_gauss(seed, gs, f, j, q); a field whose
 *             sigma is exactly 0 is copied (sp is 0 where both its coefficients are, whatever a.a)
 * Afterwards frame[s] = f + 1. A car's draws depend on (seed, gs, f, j) only: shards concatenate. */
#define PP_SENSE_NONE      0   /* fate of a row r >= n_cars[s]: no truth row                       */
#define PP_SENSE_REPORTED  1
#define PP_SENSE_OCCLUDED  2
#define PP_SENSE_DROPPED   3

typedef struct pp_sensor_cfg {
    uint64_t seed;
    int64_t  first_scene;          /* global index of the batch's scene 0 (shards), >= 0            */
    double   pos_sigma;            /* 0 m: position noise at the ego                                */
    double   pos_sigma_per_m;      /* 0: position noise added per metre of distance                 */
    double   vel_sigma;            /* 0 m/s                                                         */
    double   dropout_prob;         /* 0: probability that a visible car is not reported, in [0, 1]  */
    double   occlusion_radius;     /* 0 m: off                                                      */
} pp_sensor_cfg;                   /* sigmas and radius finite and >= 0; the default: the identity  */

/* Sensor state of a batch (SoA, caller owned; device resident for pp_sense_frame and
 * pp_rollout_sensed, host memory for pp_sense_frame_host), S = the telemetry's n_scenes; row arrays
 * [r * S + s] for r < the telemetry's car_stride. A zero `frame` is a fresh episode and a state is
 * reused by zeroing `frame` alone. Every fate entry is written by every call; sensed rows at and
 * beyond n_cars[s] are not. */
typedef struct pp_sensor {
    int32_t* frame;                /* carried: frames sensed so far in the episode                  */
    int32_t* n_cars;               /* sensed rows                                                   */
    int32_t* car_id;               /* the sensed rows, in truth order (ascending id)                */
    double*  car_x;
    double*  car_y;
    double*  car_vx;
    double*  car_vy;
    int32_t* fate;                 /* per TRUTH row r: PP_SENSE_*                                   */
} pp_sensor;

void    pp_sensor_cfg_default(pp_sensor_cfg* c);
/* Senses ONE frame from the telemetry alone (no map), for callers with their own loop: hand pp_eval a
 * copy of the telemetry struct whose n_cars and car_* are the state's. Writes `state` only. PP_ERR_ARG
 * (before any HIP call) for a NULL argument or array, a sigma or radius that is negative or not
 * finite, a probability outside [0, 1], first_scene < 0, n_scenes < 0 or a car_stride outside
 * 0..PP_MAX_CARS. Device pointers; asynchronous on hip_stream. */
int32_t pp_sense_frame(const pp_scene_batch* telemetry, const pp_sensor_cfg* cfg, pp_sensor* state,
                       int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_sense_frame_host(const pp_scene_batch* telemetry, const pp_sensor_cfg* cfg, pp_sensor* state);
/* The draws restated on the host (bit-identical to the device's): Gaussian q = 0..3 (x, y, vx, vy)
 * and the dropout word of car `car` in frame `frame` of global scene `scene`. Philox4x32-10, key =
 * seed, counter = {scene lo, scene hi, (frame PP_NOISE_CAR_STRIDE + car) 8 + q, 0x53454E53} (mod 2^32;
 * the dropout block is q = 4, its word 0); the Gaussian is pp_mc_gauss's Irwin-Hall unit. */
double  pp_sensor_gauss(uint64_t seed, int64_t scene, int32_t frame, int32_t car, int32_t q);
uint32_t pp_sensor_word(uint64_t seed, int64_t scene, int32_t frame, int32_t car);
/* pp_rollout_lane_changing with the sensor: a frame begins with the sensor on the telemetry, pp_eval
 * plans from the sensed rows (and updates the telemetry's car table from them, so a car that is not
 * reported keeps its stale entry), and the follow update, the lane changes, the judge and the
 * simulator read and write the truth as before. The log's n_cars is the truth's. scfg and sstate both
 * NULL: exactly pp_rollout_lane_changing; one alone is refused. */
int32_t pp_rollout_sensed(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                          const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                          pp_rollout_log* log, int32_t device, void* hip_stream,
                          const pp_judge_cfg* jcfg, pp_judge* jstate,
                          const pp_follow_cfg* fcfg, pp_follow* fstate,
                          const pp_lane_change_cfg* lcfg, pp_lane_change* lstate,
                          const pp_sensor_cfg* scfg, pp_sensor* sstate);
/* pp_rollout_sweep with a sensor per set: set p is driven with sets[p] and sensor_sets[p] (host
 * memory, n_sets entries). Per set the steps are pp_rollout_sweep's, but sstate->frame is zeroed on
 * the stream before the drive, and the drive is pp_rollout_sensed. Every set is checked before the
 * first launch. */
int32_t pp_rollout_sweep_sensed(pp_map* m, const pp_params* sets, const pp_sweep_cfg* cfg,
                                const pp_episode_cfg* ecfg, const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg,
                                const pp_lane_change_cfg* lcfg, pp_scene_batch* telemetry, pp_traffic* traffic,
                                pp_result* result, pp_judge* jstate, pp_follow* fstate, pp_lane_change* lstate,
                                pp_judge_stats* stats, int32_t device, void* hip_stream,
                                const pp_sensor_cfg* sensor_sets, pp_sensor* sstate);

/* ---- tracker: one Kalman filter per sensed car, between the sensor and the planner ------------- */
/* Sensor fusion gives stable ids, so there is no assignment: per scene the tracker merges its old
 * tracks with the frame's rows in id order. A car in both is filtered (constant velocity, position
 * and velocity measured, one 2x2 covariance shared by both axes), a car only in the rows starts a
 * track at its report, a car only in the tracks coasts on its predicted straight line for up to
 * max_coast frames and is then deleted. THIS LIBRARY'S OWN definitions (DESIGN.md "Tracker" and
 * csrc/pp_tracker.h state every formula and its operation order). No gating, no confirmation, no map.
 * The rows are `seen`'s ego_x, ego_y, n_cars and car rows (the telemetry with a sensor state's rows in
 * place, or the plain truth), only read: n = clamp(n_cars[s], 0, K), K = seen->car_stride; rows are
 * expected in ascending id and a row whose id is <= the last accepted row's is skipped. A coasting
 * track is also deleted where it would leave no room for the rows still to come (reported rows always
 * fit); with max_coast and every sigma 0 (the default) the tracked rows are the accepted rows bit for
 * bit. dt = consume x 0.02 s. */
#define PP_TRACK_NONE      0   /* src of a row r >= n_cars[s]: no track                            */
#define PP_TRACK_NEW       1   /* first report of the id: the report itself                         */
#define PP_TRACK_UPDATED   2   /* prediction corrected by the report                                */
#define PP_TRACK_COASTED   3   /* not reported: the prediction                                      */

typedef struct pp_tracker_cfg {
    double  meas_pos_sigma;        /* 0 m: the filter's model of the sensor's pos_sigma             */
    double  meas_pos_sigma_per_m;  /* 0: ... of its pos_sigma_per_m                                 */
    double  meas_vel_sigma;        /* 0 m/s: ... of its vel_sigma                                   */
    double  acc_sigma;             /* 0 m/s^2: process noise (white acceleration)                   */
    int32_t max_coast;             /* 0: frames a track outlives its last report, >= 0              */
    int32_t _pad;
} pp_tracker_cfg;                  /* sigmas finite and >= 0; the default: the identity tracker     */

/* Tracker state of a batch (SoA, caller owned; device resident for pp_track_frame and
 * pp_rollout_tracked, host memory for pp_track_frame_host), S = seen->n_scenes, K = seen->car_stride.
 * Two banks of K track slots, field [(b * K + k) * S + s], n_tracks[b * S + s]: with f = frame[s] a
 * call reads bank f & 1 and writes the other. Where f == 0 the old bank counts as empty whatever it
 * holds, so a state is reused by zeroing `frame` alone. The tracked rows [r * S + s] (the new bank's
 * tracks, ascending id) and src are written, never read; every src entry is written by every call,
 * rows at and beyond n_cars[s] are not. */
typedef struct pp_tracker {
    int32_t* frame;                /* [S] carried: frames tracked so far in the episode             */
    int32_t* n_tracks;             /* [2 S]                                                         */
    int32_t* id;                   /* [2 K S] the banks                                             */
    int32_t* misses;               /*         frames since the last report                          */
    double*  x;
    double*  y;
    double*  vx;
    double*  vy;
    double*  ppp;                  /*         covariance: position, position-velocity, velocity     */
    double*  ppv;
    double*  pvv;
    int32_t* n_cars;               /* [S] tracked rows                                              */
    int32_t* car_id;               /* [K S] the tracked rows: what pp_eval is handed                */
    double*  car_x;
    double*  car_y;
    double*  car_vx;
    double*  car_vy;
    int32_t* src;                  /* [K S] per tracked row: PP_TRACK_*                             */
} pp_tracker;

void    pp_tracker_cfg_default(pp_tracker_cfg* c);
/* Tracks ONE frame (no map), for callers with their own loop: hand pp_eval a copy of the telemetry
 * struct whose n_cars and car_* are the state's. Writes `state` only. PP_ERR_ARG (before any HIP call)
 * for a NULL argument or array, n_scenes < 0, a car_stride outside 0..PP_MAX_CARS, consume < 1, a
 * sigma that is negative or not finite, max_coast < 0. Device pointers; asynchronous on hip_stream. */
int32_t pp_track_frame(const pp_scene_batch* seen, const pp_tracker_cfg* cfg, int32_t consume,
                       pp_tracker* state, int32_t device, void* hip_stream);
/* The same on the host (host pointers; the same arithmetic, bit for bit). */
int32_t pp_track_frame_host(const pp_scene_batch* seen, const pp_tracker_cfg* cfg, int32_t consume,
                            pp_tracker* state);
/* pp_rollout_sensed with the tracker: a frame is the sensor on the telemetry (where asked for), the
 * tracker on the sensed rows (on the truth rows without a sensor), then pp_eval on the tracked rows
 * (it updates the telemetry's car table from them); every other stage reads and writes the truth and
 * the log's n_cars is the truth's. tcfg and tstate both NULL: exactly pp_rollout_sensed; one alone is
 * refused. */
int32_t pp_rollout_tracked(pp_map* m, pp_scene_batch* telemetry, pp_traffic* traffic,
                           const pp_params* prm, const pp_rollout_cfg* cfg, pp_result* result,
                           pp_rollout_log* log, int32_t device, void* hip_stream,
                           const pp_judge_cfg* jcfg, pp_judge* jstate,
                           const pp_follow_cfg* fcfg, pp_follow* fstate,
                           const pp_lane_change_cfg* lcfg, pp_lane_change* lstate,
                           const pp_sensor_cfg* scfg, pp_sensor* sstate,
                           const pp_tracker_cfg* tcfg, pp_tracker* tstate);
/* pp_rollout_sweep_sensed with a tracker per set: set p is driven with sets[p], sensor_sets[p] and
 * tracker_sets[p] (host memory, n_sets entries each). Per set sstate->frame and tstate->frame are
 * zeroed on the stream before the drive, and the drive is pp_rollout_tracked. Every set is checked
 * before the first launch. */
int32_t pp_rollout_sweep_tracked(pp_map* m, const pp_params* sets, const pp_sweep_cfg* cfg,
                                 const pp_episode_cfg* ecfg, const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg,
                                 const pp_lane_change_cfg* lcfg, pp_scene_batch* telemetry, pp_traffic* traffic,
                                 pp_result* result, pp_judge* jstate, pp_follow* fstate, pp_lane_change* lstate,
                                 pp_judge_stats* stats, int32_t device, void* hip_stream,
                                 const pp_sensor_cfg* sensor_sets, pp_sensor* sstate,
                                 const pp_tracker_cfg* tracker_sets, pp_tracker* tstate);

/* A batch in HOST memory (the batched onMessage; what a server calls per tick): stages the
 * scenes — and their car table when tab_valid is set, updated in place — through device memory,
 * runs pp_eval on hip_stream and copies winner, n_out, next_x/next_y, cost and status back into
 * the host pp_result. Synchronous. emit_paths must be 0. */
int32_t pp_plan_batch_host(pp_map* m, int32_t device, pp_scene_batch* host_in, const pp_params* prm,
                           pp_result* host_out, void* hip_stream);

/* pp_plan_frame keeps the reference's car table across calls (per map and device, any ids);
 * pp_plan_reset empties it (a new episode). */
int32_t pp_plan_reset(pp_map* m, int32_t device);

/* ---- simulator wire codec (host code) ----------------------------- */
/* Parses n_msgs socket.io frames `42["telemetry",{...}]` — message m is buf[offsets[m],
 * offsets[m+1]) — into scenes [0, n_msgs) of a HOST batch (out->n_scenes >= n_msgs), exactly as
 * the reference's hasData (helpers.h:15-25) + nlohmann::json parse and field reads
 * (src/main.cpp:1217-1252, 1325-1333) see them: previous_path_x/_y keep their first 10 points and
 * n_prev = their length; sensor_fusion rows in std::map order (ascending id, last row of an id
 * wins). msg_status[m]: 0 telemetry; 1 no data (hasData empty: the reference answers
 * `42["manual",{}]`); 2 telemetry with more distinct cars than car_stride (the first car_stride
 * kept); 3 no "42" prefix or another event (the reference does not answer); -1 malformed (the
 * reference's json::parse or field reads would throw). n_threads host threads (<= 1: the calling
 * thread). */
int32_t pp_telemetry_parse(const char* buf, const int64_t* offsets, int64_t n_msgs, pp_scene_batch* out,
                           int32_t* msg_status, int32_t n_threads);
/* Formats `42["control",{"next_x":[...],"next_y":[...]}]` per scene from HOST next_x/next_y
 * ([i * stride + s], the pp_result layout with stride = n_scenes of the batch) and n_out, as
 * nlohmann::json dump does (%.15g, ".0" for integral values, null for non-finite;
 * src/main.cpp:1461-1464). Message s is out[offsets[s], offsets[s+1]). Returns PP_ERR_NOMEM with
 * offsets[n_scenes] = bytes needed when out_cap is too small. */
int32_t pp_control_format(const double* next_x, const double* next_y, const int32_t* n_out, int64_t n_scenes,
                          int64_t stride, char* out, int64_t out_cap, int64_t* offsets, int32_t n_threads);

/* The same codec on the GPU (one lane per frame; identical parser, number conversions and
 * writer). d_buf: the frames back to back in device memory, 16-byte aligned and readable up to
 * offsets[n] rounded up to 16; d_out: a DEVICE batch (n_scenes >= n_msgs). Statuses as above,
 * plus 4: the frame needs the host codec (a number outside the exact conversions' domain, or more
 * sensor_fusion rows than the batch's car_stride) — its fields are not written. Frames of any
 * number of rows up to car_stride parse on the device. Asynchronous on hip_stream. */
int32_t pp_telemetry_parse_device(const char* d_buf, const int64_t* d_offsets, int64_t n_msgs, pp_scene_batch* d_out,
                                  int32_t* d_status, int32_t device, void* hip_stream);
/* Control messages on the GPU into fixed slots: message s = d_slots[s * slot_bytes, + d_len[s]);
 * d_len[s] = -1 when the host codec must format it (a number outside fmt15g's domain, or the
 * slot too small). slot_bytes a multiple of 16; d_slots 16-byte aligned. Asynchronous. */
int32_t pp_control_format_device(const double* d_next_x, const double* d_next_y, const int32_t* d_n_out,
                                 int64_t n_scenes, int64_t stride, char* d_slots, int64_t slot_bytes,
                                 int32_t* d_len, int32_t device, void* hip_stream);

/* ---- simulator shim (host code) ------------------------------------ */
/* A WebSocket server that speaks what the reference's uWS hub speaks on port 4567
 * (src/main.cpp:1214-1494): text frames with socket.io events; per frame the lambda's answers
 * (telemetry -> `42["control",...]`, a "42" frame without data -> `42["manual",{}]`, anything
 * else -> none). Every tick it takes one pending frame from each connected client and plans all of
 * them in one pp_plan_batch_host call (reference decision, 3 x n_speeds candidates); each
 * connection keeps the lambda's cross-frame state (car table, target_lane = 1 at start). */
typedef struct pp_server_opts {
    const char* host;              /* "127.0.0.1" (NULL: same)                                    */
    int32_t port;                  /* 4567 in the reference; 0 = any free port (see bound_port)    */
    int32_t max_clients;           /* connections served (and batched) at once                     */
    int32_t n_speeds;              /* 1 = the reference's own 3 candidates                         */
    int32_t threads;               /* codec threads                                                */
    int32_t device;
    int32_t _pad;
    int64_t max_frames;            /* return after this many telemetry frames (0: until *stop)     */
} pp_server_opts;

/* Blocking; returns when *stop != 0 (set from another thread) or after max_frames. bound_port
 * receives the listening port once bound; stats (4): telemetry frames, batches, connections
 * accepted, replies sent. */
int32_t pp_serve(pp_map* m, const pp_server_opts* opts, volatile int32_t* stop, int32_t* bound_port,
                 int64_t* stats);
/* RFC 6455 Sec-WebSocket-Accept for a client key (the handshake's known-answer check). */
int32_t pp_ws_accept_key(const char* key, char* out, int32_t cap);

/* Debug switches (process-wide; tests and A/B measurements only). Every key defaults to 0, the
 * library's own choice; results never depend on them (the tests check that bit for bit).
 *   PP_DBG_PREP_GROUP  lanes per evaluation of the scene-preparation kernel K1: 1, 2, 4, 8, 16
 *   PP_DBG_PREP_WAVES  K1's one-lane build: 3 or 4 waves per SIMD
 *   PP_DBG_SHAPE       reference-mode launch shape: PP_SHAPE_SPLIT (k_prep, k_cand, k_emit),
 *                      PP_SHAPE_CAND_SMALL (K1, then K2 + K4 in one launch), PP_SHAPE_STEP (the
 *                      whole step in one launch, small batches)
 *   PP_DBG_POISON      1: every call starts from NaN-filled intermediate buffers (prep workspace,
 *                      winner record, staging copies, new car-table slots) and checks that the
 *                      slow-group bitmap is all zero (PP_ERR_STATE otherwise), so no kernel can pass
 *                      a test on what an earlier call left behind
 *   PP_DBG_SPLIT       multi-stream split of reference-mode batches (2 or 3 parts, each K1 -> K2 ->
 *                      K4 on its own stream; beyond 1,572,864 scenes ceil(S / 1,048,576) sequential
 *                      chunks, at most 4 (so chunks of more than 1,048,576 scenes beyond 4,194,304),
 *                      3 parts each): 1 on for every batch the split can take (reference
 *                      mode without paths or draws, more than 65,536 scenes, at least 2,048), 2 off
 *                      (0: batches of 131,072 scenes and more)
 *   PP_DBG_LAST_PARTS  read-only: the parts the last pp_eval launched, 1 when not split
 *   PP_DBG_SORT_CARS   1: order each scene's cars in a pre-pass (k_sort_cars) so the one-lane K1
 *                      reads them visit-major (coalesced; same results, less fetched, slower),
 *                      2 or 0: K1 sorts and gathers them itself (the default)
 *   PP_DBG_PERSIST     the persistent K2 of reference mode without paths or draws on one stream
 *                      (resident blocks that claim their groups from a counter): 1 on for every
 *                      such batch, 2 off (0: batches of more than 1,572,864 scenes)
 *   PP_DBG_LAST_PERSIST read-only: the resident block count of the last pp_eval's persistent K2
 *                      (its grid is that, or one block per group if fewer), 0 when it ran none
 *   PP_DBG_LAST_PERSIST_SHAPE read-only: 1 when that persistent K2 was the instantiation with
 *                      BASELINE config 5's shape as compile-time constants (5 speeds, 3 lanes, 17
 *                      scenes per group in 256 threads; taken at 50 points), 0 when it was the
 *                      generic one or none ran
 * Returns PP_ERR_ARG for an unknown key or value. */
#define PP_DBG_PREP_GROUP  0
#define PP_DBG_PREP_WAVES  1
#define PP_DBG_SHAPE       2
#define PP_DBG_POISON      3
#define PP_DBG_SPLIT       4
#define PP_DBG_LAST_PARTS  5
#define PP_DBG_SORT_CARS   6
#define PP_DBG_PERSIST     7
#define PP_DBG_LAST_PERSIST 8
#define PP_DBG_LAST_PERSIST_SHAPE 9
#define PP_DBG_KEYS        10
#define PP_SHAPE_SPLIT      1
#define PP_SHAPE_CAND_SMALL 2
#define PP_SHAPE_STEP       3
int32_t pp_debug_set(int32_t key, int32_t value);
int32_t pp_debug_get(int32_t key);

/* Per-kernel timing with HIP events recorded on the launch stream around every kernel of pp_eval
 * (K1 k_prep, K2 k_cand, K3/K4 k_winner or k_emit; a split call (PP_DBG_SPLIT) times each part on
 * its own stream and counts each stage once, as the span from its earliest part's start to its
 * latest part's end: the parts overlap). enable PP_TIMING_K2 records only K2's two
 * events per launch (an event costs a few microseconds of stream time: the bench's timed region
 * records only what its roofline needs); any other nonzero value, every kernel's. pp_timing_read
 * synchronises on the recorded events, returns the summed milliseconds and launch counts per kernel
 * (k_prep and k_winner/k_emit 0 launches under PP_TIMING_K2), and clears the record. */
#define PP_TIMING_ALL 1
#define PP_TIMING_K2  2
int32_t pp_timing_enable(pp_map* m, int32_t device, int32_t enable);
int32_t pp_timing_read(pp_map* m, int32_t device, double* ms3, int64_t* launches3);

/* The Monte-Carlo noise generator (host copy of the device code; bit-identical): standard-normal-
 * like variate q (0..3 -> x, y, vx, vy) of car j in draw d of global scene `scene`. Irwin-Hall of
 * four 32-bit Philox4x32-10 uniforms (key = seed, counter = {scene, (d*PP_NOISE_CAR_STRIDE + j)*4 + q,
 * 0x4D43}), scaled to unit variance: only exactly rounded arithmetic, no libm. */
double  pp_mc_gauss(uint64_t seed, int64_t scene, int32_t draw, int32_t car, int32_t q);

/* The reference's libm as the kernels compute it (csrc/pp_glibcm.h: glibc 2.35 x86-64 sin, cos,
 * atan2 restated bit for bit; used for the frame's heading and rotations in k_prep, the device
 * Map::Init and the scene generator). Evaluates out[i] = sin(a[i]) (kind 0), cos(a[i]) (kind 1) or
 * atan2(a[i], b[i]) (kind 2) for i < n on `device` (pointers to device memory, on `hip_stream`),
 * or on the host (device = -1, host pointers). sin/cos outside |x| < 105414350 give NaN. For
 * parity tests of the device build against the host libm. */
int32_t pp_libm_eval(int32_t kind, const double* a, const double* b, double* out, int64_t n,
                     int32_t device, void* hip_stream);

/* The candidate loop's FP64 primitives over arrays (csrc/pp_math.h, the SpeedController wrappers of
 * csrc/pp_device.h, the turn functions of csrc/pp_k_frame.h), each kind calling the function the
 * loop calls: for tests/test_math_primitives.py, which holds every primitive's written accuracy
 * claim against an exact reference. Every pointer is device memory on `device` (>= 0), work goes
 * to `hip_stream`; inputs and outputs a kind does not use are null; booleans pass as 0.0 / 1.0.
 *   kind                                  in                          out
 *   SINCOS, SINCOS_NOLARGE                a                           sin, cos   (sincos_pp<true/false>)
 *   ATAN2_PP, ATAN2_FAST, ATAN2_UNIT      a = y, b = x                angle
 *   ASIN_SMALL, RCP_NR                    a                           value
 *   DIV_RCP, DIV_RCP_NC                   a = n, b = d, c = r         quotient
 *   DIV_RCP_AUTO, DIV_RCP_NC_AUTO         a = n, b = d                quotient   (r = rcp_nr(d) inside)
 *   DIV50, DIV50_NC                       a                           div_rcp(a, 50, 0.02), div50_nc(a)
 *   SQRT_RD                               a                           d, rd, dok
 *   DIV_RCP_N, DIV_RCP_D                  a = n, b = q                n / sqrt(q)  (sqrt_rd(q) first)
 *   FMOD_2PI, FMOD_2PI_SMALL              a                           remainder
 *   TURN_SINCOS, TURN_SINCOS_NOLARGE      a                           sin, cos   (turn_sincos<true/false>)
 *   SINCOS_SMALL                          a                           sin, cos
 *   TURN_ANGLE, _NOLARGE, _FAST           a = nc, b = speed, c = adiff  rot      (turn_angle<true/false>, turn_angle_fast)
 *   SC_SPEED, SC_SPEED_R, SC_SPEED_R_NC   a, b, c = start, target, ttime; d = 2 planes of n: shift, k
 *                                         speed at t = 0.02 k (sc_get_speed; sc_get_speed_r<true/false>
 *                                         with r = rcp_nr(ttime))
 *   SC_OVERRIDE, _R, _R_NC                a, b, c as above; d = 3 planes of n: shift, k, speed
 *                                         the new shift (sc_override; sc_override_r<true/false> with
 *                                         r = rcp_nr(target - start))
 *   SPEED_IN_RANGE                        a                           0 / 1
 * A bad kind, a missing array, n < 0 or a bad device: PP_ERR_ARG; n = 0: PP_OK. */
enum {
    PP_MATH_SINCOS = 0, PP_MATH_SINCOS_NOLARGE, PP_MATH_ATAN2_PP, PP_MATH_ATAN2_FAST, PP_MATH_ATAN2_UNIT,
    PP_MATH_ASIN_SMALL, PP_MATH_RCP_NR, PP_MATH_DIV_RCP, PP_MATH_DIV_RCP_NC, PP_MATH_DIV_RCP_AUTO,
    PP_MATH_DIV_RCP_NC_AUTO, PP_MATH_DIV50, PP_MATH_DIV50_NC, PP_MATH_SQRT_RD, PP_MATH_DIV_RCP_N,
    PP_MATH_DIV_RCP_D, PP_MATH_FMOD_2PI, PP_MATH_FMOD_2PI_SMALL, PP_MATH_TURN_SINCOS,
    PP_MATH_TURN_SINCOS_NOLARGE, PP_MATH_SINCOS_SMALL, PP_MATH_TURN_ANGLE, PP_MATH_TURN_ANGLE_NOLARGE,
    PP_MATH_TURN_ANGLE_FAST, PP_MATH_SC_SPEED, PP_MATH_SC_SPEED_R, PP_MATH_SC_SPEED_R_NC,
    PP_MATH_SC_OVERRIDE, PP_MATH_SC_OVERRIDE_R, PP_MATH_SC_OVERRIDE_R_NC, PP_MATH_SPEED_IN_RANGE,
    PP_MATH_KINDS
};
int32_t pp_math_eval(int32_t kind, const double* a, const double* b, const double* c, const double* d,
                     double* out0, double* out1, double* out2, int64_t n, int32_t device, void* hip_stream);

/* Library version / build info string. */
const char* pp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PP_H */
