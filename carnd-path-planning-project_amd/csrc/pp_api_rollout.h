// pp_api_rollout.h — host: closed-loop rollouts, the judge, reactive traffic, the sensor model, the
// tracker, the judge summary and parameter sweeps (C ABI).
// Part of pp_eval.hip's translation unit.
#pragma once

namespace {
// one frame of a world stage on the device (W: the device views); each returns launch_scenes' code
int launch_judge(const WorldTables& W, const pp_scene_batch* tel, const ppsynth::TrafficV& tv, const pp_result* plan,
                 int32_t consume, const pp_judge_cfg* jc, const pp_judge* js, void* stream) {
    return launch_scenes(k_judge, tel->n_scenes, stream, W.T, tel->n_scenes, tel->ego_x, tel->ego_y,
                         tel->ego_yaw_deg, plan->next_x, plan->next_y, plan->n_out, tv, consume, *jc, *js);
}

int launch_follow(const WorldTables& W, const pp_scene_batch* tel, const ppsynth::TrafficV& tv, int32_t consume,
                  const pp_follow_cfg* fc, const pp_follow* fs, void* stream) {
    return launch_scenes(k_follow, tel->n_scenes, stream, W.T, W.AT, tel->n_scenes, tel->ego_x, tel->ego_y,
                         tel->ego_speed_mph, tv, consume, *fc, *fs);
}

int launch_lane_change(const WorldTables& W, const pp_scene_batch* tel, const ppsynth::TrafficV& tv, int32_t consume,
                       const pp_follow_cfg* fc, const pp_follow* fs, const pp_lane_change_cfg* lc,
                       const pp_lane_change* ls, void* stream) {
    return launch_scenes(k_lane_change, tel->n_scenes, stream, W.T, W.AT, tel->n_scenes, tel->ego_x, tel->ego_y,
                         tel->ego_speed_mph, tv, consume, *fc, *fs, *lc, *ls);
}

int launch_sense(const pp_scene_batch* tel, const pp_sensor_cfg* sc, const pp_sensor* ss, void* stream) {
    return launch_scenes(k_sense, tel->n_scenes, stream, truth_view(tel), *sc, *ss);
}

int launch_track(const pp_scene_batch* seen, const pp_tracker_cfg* tc, int32_t consume, const pp_tracker* ts,
                 void* stream) {
    return launch_scenes(k_track, seen->n_scenes, stream, truth_view(seen), *tc, consume * 0.02, *ts);
}

// `b` with the rows of a sensor or tracker state in place of its own (the other arrays shared)
template <class State>
pp_scene_batch with_rows(const pp_scene_batch& b, const State& x) {
    pp_scene_batch v = b;
    v.n_cars = x.n_cars; v.car_id = x.car_id;
    v.car_x = x.car_x; v.car_y = x.car_y;
    v.car_vx = x.car_vx; v.car_vy = x.car_vy;
    return v;
}

// every argument check of pp_synth_episode and its host twin (no HIP call); *gap: the gap rule in force
bool episode_ok(const pp_map* M, int64_t first_scene, const pp_episode_cfg* cfg, const pp_follow_cfg* gap_rule,
                const pp_scene_batch* tel, const pp_traffic* traffic, const pp_judge* js, const pp_follow* fs,
                pp_follow_cfg* gap) {
    if (!M || !cfg || !tel || !traffic || first_scene < 0 || tel->n_scenes < 0) return false;
    if (!tel->ego_x || !tel->ego_y || !tel->ego_yaw_deg || !tel->ego_speed_mph || !tel->prev_x || !tel->prev_y ||
        !tel->n_prev || !tel->prev_target_lane || !tel->n_cars || !tel->car_id || !tel->car_x || !tel->car_y ||
        !tel->car_vx || !tel->car_vy)
        return false;
    if (!traffic->lane || !traffic->seg || !traffic->t || !traffic->offset || !traffic->speed) return false;
    if ((js && !judge_state_ok(js)) || (fs && !follow_state_ok(fs))) return false;
    if (!ppepisode::cfg_ok(*cfg) || cfg->n_cars > tel->car_stride) return false;
    if (tel->tab_valid && (tel->tab_slots < cfg->n_cars || tel->tab_slots > PP_MAX_CARS)) return false;
    if (gap_rule) *gap = *gap_rule; else ppfollow::cfg_default(gap);
    // (the follow update takes any headway and standstill gap; a placement by them needs numbers >= 0)
    if (!ppfollow::cfg_ok(*gap) || !(gap->time_headway >= 0) || !(gap->min_gap >= 0)) return false;
    const ppfollow::ArcTables A = host_tables(M).AT;
    double min_loop = A.loop[0];
    for (int l = 1; l < PP_NUM_LANES; l++) min_loop = A.loop[l] < min_loop ? A.loop[l] : min_loop;
    return ppepisode::ring_ok(*cfg, *gap, min_loop);
}

// The rollout's optional stages. A stage is asked for by its configuration or its state, and then
// needs both; `need`: the stages the entry point cannot do without.
enum : int { kJudge = 1, kFollow = 2 };
struct Stages {
    int need = 0;
    const pp_judge_cfg* jc = nullptr;
    const pp_judge* js = nullptr;
    const pp_follow_cfg* fc = nullptr;
    const pp_follow* fs = nullptr;
    const pp_lane_change_cfg* lc = nullptr;
    const pp_lane_change* ls = nullptr;
    const pp_sensor_cfg* sc = nullptr;
    const pp_sensor* ss = nullptr;
    const pp_tracker_cfg* tc = nullptr;
    const pp_tracker* ts = nullptr;
};

// each stage asked for against its own arguments and what it reads of a frame; lane changes read the
// follow update's records, so they need that stage
bool stages_ok(const Stages& st, const pp_scene_batch* tel, const pp_traffic* traffic, const pp_result* res,
               int32_t consume) {
    const bool judge = st.jc || st.js, follow = st.fc || st.fs, change = st.lc || st.ls, sense = st.sc || st.ss;
    const bool track = st.tc || st.ts;
    if (((st.need & kJudge) && !judge) || ((st.need & kFollow) && !follow)) return false;
    if (judge && (!judge_ok(st.jc, st.js) || !judge_frame_ok(tel, traffic, res, consume))) return false;
    if (follow && (!follow_ok(st.fc, st.fs) || !follow_frame_ok(tel, traffic, consume))) return false;
    if (sense && (!sense_frame_ok(tel) || !sensor_ok(st.sc, st.ss, tel->car_stride))) return false;
    if (track && (!sense_frame_ok(tel) || !tracker_ok(st.tc, st.ts, tel->car_stride) || consume < 1)) return false;
    return !change || (follow && lane_change_ok(st.lc, st.ls));
}

// every argument check of rollout_loop (no HIP call)
bool rollout_ok(const pp_map* M, const pp_scene_batch* tel, const pp_traffic* traffic, const pp_params* prm,
                const pp_rollout_cfg* cfg, const pp_result* res, const pp_rollout_log* log, int32_t device,
                const Stages& st) {
    if (!M || !tel || !prm || !cfg || !res || device < 0 || device >= kMaxDev || !traffic_ok(traffic, tel) ||
        !stages_ok(st, tel, traffic, res, cfg->consume))
        return false;
    if (cfg->n_frames < 0 || cfg->consume < 1 || !(cfg->sensor_range >= 0) || prm->n_draws > 1 ||
        prm->emit_paths || !tel->tab_valid || !tel->tab_lane || !tel->tab_s || !tel->tab_d ||
        !tel->tab_vs || !tel->tab_vd || !tel->tab_vx || !tel->tab_vy || tel->car_stride < traffic->n_cars ||
        tel->tab_slots < traffic->n_cars)
        return false;
    return !(log && log->plan_x && !log->plan_y);
}

// pp_rollout's loop, a frame in this order: k_sense, k_track, pp_eval, k_follow, k_lane_change (not
// without cars), k_judge, k_sim, each of the five only where its stage is asked for. With the sensor
// `sensed` is the telemetry with the sensor state's rows in place of the truth's; with the tracker
// pp_eval plans from `seen`, the telemetry with the tracker's rows (made from `sensed`), otherwise from
// `sensed` itself (the car table is shared, so it is updated as before); every other stage reads and
// writes the truth.
int32_t rollout_loop(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                     const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                     void* hip_stream, const Stages& st) {
    if (!rollout_ok(M, tel, traffic, prm, cfg, res, log, device, st)) return PP_ERR_ARG;
    if (tel->n_scenes == 0 || cfg->n_frames == 0) return PP_OK;
    const WorldDev W(M, device, st.fs != nullptr);      // (the arc prefix: the follow stage's)
    if (W.rc) return W.rc;
    SimArgs A;
    A.consume = cfg->consume;
    A.range2 = cfg->sensor_range * cfg->sensor_range;
    if (log) A.log = *log; else memset(&A.log, 0, sizeof(A.log));
    const ppsynth::TrafficV tv = traffic_view(traffic, tel->n_scenes);
    const pp_scene_batch sensed = st.ss ? with_rows(*tel, *st.ss) : *tel;
    const pp_scene_batch seen = st.ts ? with_rows(*tel, *st.ts) : sensed;
    for (int f = 0; f < cfg->n_frames; f++) {
        int rc = st.ss ? launch_sense(tel, st.sc, st.ss, hip_stream) : PP_OK;
        if (rc == PP_OK && st.ts) rc = launch_track(&sensed, st.tc, cfg->consume, st.ts, hip_stream);
        if (rc == PP_OK) rc = pp_eval(M, &seen, prm, res, device, hip_stream);
        if (rc == PP_OK && st.fs) rc = launch_follow(W, tel, tv, cfg->consume, st.fc, st.fs, hip_stream);
        if (rc == PP_OK && st.ls && tv.n > 0)
            rc = launch_lane_change(W, tel, tv, cfg->consume, st.fc, st.fs, st.lc, st.ls, hip_stream);
        if (rc == PP_OK && st.js) rc = launch_judge(W, tel, tv, res, cfg->consume, st.jc, st.js, hip_stream);
        A.frame = f;
        if (rc == PP_OK) rc = launch_scenes(k_sim, tel->n_scenes, hip_stream, W.T, *tel, tv, *prm, *res, A);
        if (rc != PP_OK) return rc;
    }
    return PP_OK;
}

// every argument check of pp_judge_summary and its host twin (no HIP call)
bool summary_ok(const pp_judge* js, int64_t S, const pp_summary_cfg* c, const pp_judge_stats* o) {
    return c && judge_state_ok(js) && ppsummary::stats_ok(o) && ppsummary::cfg_ok(*c, S);
}

// The summary's launch geometry (no HIP call): false where a grid would not fit.
bool summary_args(int64_t S, const pp_summary_cfg& c, SumArgs& A) {
    A.S = S; A.E = c.scenes_per_group; A.G = ppsummary::n_groups(S, A.E);
    A.tpg = ppsummary::n_tiles(A.E < S ? A.E : S);
    A.R = c.out_stride ? c.out_stride : A.G; A.out_first = c.out_first;
    A.B = c.hist_bins; A.inv_w = c.hist_bins / c.hist_max;
    A.direct = A.tpg == 1;
    if (A.G > 0x7fffffff || A.tpg > 0x7fffffff || A.G * A.tpg > 0x7fffffff || (A.G * A.B + 255) / 256 > 0x7fffffff)
        return false;
    // tiles per chunk: as many as leave kSumBlocks blocks or more, at most kSumChunkMax (1,024 blocks of
    // 8 tiles at 2,097,152 scenes: four resident blocks on each of 256 CUs); no figure depends on it
    constexpr int64_t kSumBlocks = 512;
    const int64_t k = A.G * A.tpg / kSumBlocks;
    A.K = (int)(k < 1 ? 1 : (k > kSumChunkMax ? kSumChunkMax : k));
    if (A.K > A.tpg) A.K = A.tpg > 0 ? (int)A.tpg : 1;    // (no scenes: no tiles)
    A.cpg = (A.tpg + A.K - 1) / A.K;
    return true;
}

// k_summary_clear, k_summary_tiles and, for groups of more than one tile, k_summary_groups over the
// records of the stream's workspace (the chunks' parts, then T_t of the two sums per tile; grown under
// M->mu, which is held through the launches as in pp_eval); arguments checked by the caller
int launch_summary(pp_map* M, const pp_judge* js, const SumArgs& A, const pp_judge_stats* o, int32_t device,
                   void* hip_stream) {
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t blocks = A.G * A.cpg, tiles = A.G * A.tpg;
    DeviceGuard g(device);
    std::lock_guard<std::mutex> lk(M->mu);
    SumRecs rec = {nullptr, nullptr, nullptr};
    if (!A.direct) {
        DevMem<>& W = M->dev[device].sws[hip_stream].sum;
        const size_t bytes = sizeof(ppsummary::Part) * (size_t)blocks + 2 * sizeof(double) * (size_t)tiles;
        const int rc = W.grow(st, (int64_t)bytes, bytes);
        if (rc) return rc;
        rec.part = (ppsummary::Part*)W.get();
        rec.td = (double*)(rec.part + blocks);
        rec.tc = rec.td + tiles;
    }
    hipLaunchKernelGGL(k_summary_clear, dim3((unsigned)((A.G * A.B + 255) / 256)), dim3(256), 0, st, A, o->hist);
    hipLaunchKernelGGL(k_summary_tiles, dim3((unsigned)blocks), dim3(256), 0, st, *js, A, *o, rec);
    if (!A.direct) hipLaunchKernelGGL(k_summary_groups, dim3((unsigned)A.G), dim3(256), 0, st, A, rec, *o);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

// the optional states as the episode functions take them: by value, zeroed where absent
template <class State>
State or_zero(const State* p) {
    State v;
    memset(&v, 0, sizeof(v));
    return p ? *p : v;
}
}  // namespace

extern "C" {

int32_t pp_rollout(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                   const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                   void* hip_stream) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, Stages{});
}

int32_t pp_rollout_judged(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                          const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                          void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* state) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, Stages{kJudge, jcfg, state});
}

void pp_judge_cfg_default(pp_judge_cfg* c) { if (c) ppjudge::cfg_default(c); }

int32_t pp_judge_frame(pp_map* M, const pp_scene_batch* tel, const pp_traffic* traffic, const pp_result* plan,
                       int32_t consume, const pp_judge_cfg* cfg, pp_judge* state, int32_t device,
                       void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !judge_ok(cfg, state) ||
        !judge_frame_ok(tel, traffic, plan, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    const WorldDev W(M, device, false);
    if (W.rc) return W.rc;
    return launch_judge(W, tel, traffic_view(traffic, tel->n_scenes), plan, consume, cfg, state, hip_stream);
}

int32_t pp_judge_frame_host(const pp_map* M, const pp_scene_batch* tel, const pp_traffic* traffic,
                            const pp_result* plan, int32_t consume, const pp_judge_cfg* cfg, pp_judge* state) {
    if (!M || !judge_ok(cfg, state) || !judge_frame_ok(tel, traffic, plan, consume)) return PP_ERR_ARG;
    const WorldTables W = host_tables(M);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        ppjudge::judge_scene(W.T, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_yaw_deg[s], plan->next_x,
                             plan->next_y, plan->n_out[s], tv, consume, *cfg, *state);
    return PP_OK;
}

// (a judge configuration without a judge state asks for no judge, here and in pp_rollout_lane_changing)
int32_t pp_rollout_reactive(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                            const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                            void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate,
                            const pp_follow_cfg* fcfg, pp_follow* fstate) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream,
                        Stages{kFollow, jstate ? jcfg : nullptr, jstate, fcfg, fstate});
}

void pp_follow_cfg_default(pp_follow_cfg* c) { if (c) ppfollow::cfg_default(c); }

int32_t pp_traffic_follow(pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                          const pp_follow_cfg* cfg, pp_follow* state, int32_t device, void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !follow_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    const WorldDev W(M, device, true);
    if (W.rc) return W.rc;
    return launch_follow(W, tel, traffic_view(traffic, tel->n_scenes), consume, cfg, state, hip_stream);
}

int32_t pp_traffic_follow_host(const pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                               const pp_follow_cfg* cfg, pp_follow* state) {
    if (!M || !follow_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume)) return PP_ERR_ARG;
    const WorldTables W = host_tables(M);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        ppfollow::follow_scene(W.T, W.AT, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_speed_mph[s], tv, consume,
                               *cfg, *state);
    return PP_OK;
}

void pp_lane_change_cfg_default(pp_lane_change_cfg* c) { if (c) pplanechange::cfg_default(c); }

int32_t pp_traffic_lane_change(pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                               const pp_follow_cfg* fcfg, const pp_follow* fstate, const pp_lane_change_cfg* cfg,
                               pp_lane_change* state, int32_t device, void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !follow_ok(fcfg, fstate) || !lane_change_ok(cfg, state) ||
        !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0 || traffic->n_cars == 0) return PP_OK;
    const WorldDev W(M, device, true);
    if (W.rc) return W.rc;
    return launch_lane_change(W, tel, traffic_view(traffic, tel->n_scenes), consume, fcfg, fstate, cfg, state,
                              hip_stream);
}

int32_t pp_traffic_lane_change_host(const pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                                    const pp_follow_cfg* fcfg, const pp_follow* fstate,
                                    const pp_lane_change_cfg* cfg, pp_lane_change* state) {
    if (!M || !follow_ok(fcfg, fstate) || !lane_change_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (traffic->n_cars == 0) return PP_OK;
    const WorldTables W = host_tables(M);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        pplanechange::lane_change_scene(W.T, W.AT, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_speed_mph[s], tv,
                                        consume, *fcfg, *fstate, *cfg, *state);
    return PP_OK;
}

// (a lone lcfg or a lone lstate asks for lane changes and is refused; neither: none)
int32_t pp_rollout_lane_changing(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                                 const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                                 void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate,
                                 const pp_follow_cfg* fcfg, pp_follow* fstate, const pp_lane_change_cfg* lcfg,
                                 pp_lane_change* lstate) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream,
                        Stages{kFollow, jstate ? jcfg : nullptr, jstate, fcfg, fstate, lcfg, lstate});
}

void pp_sensor_cfg_default(pp_sensor_cfg* c) { if (c) ppsensor::cfg_default(c); }

double pp_sensor_gauss(uint64_t seed, int64_t scene, int32_t frame, int32_t car, int32_t q) {
    uint32_t w[4];
    ppsensor::block(seed, (uint64_t)scene, (uint32_t)frame, (uint32_t)car, q, w);
    return ppsynth::ih_unit(w);
}

uint32_t pp_sensor_word(uint64_t seed, int64_t scene, int32_t frame, int32_t car) {
    uint32_t w[4];
    ppsensor::block(seed, (uint64_t)scene, (uint32_t)frame, (uint32_t)car, ppsensor::kDropBlock, w);
    return w[0];
}

int32_t pp_sense_frame(const pp_scene_batch* tel, const pp_sensor_cfg* cfg, pp_sensor* state, int32_t device,
                       void* hip_stream) {
    if (device < 0 || device >= kMaxDev || !sense_frame_ok(tel) || !sensor_ok(cfg, state, tel->car_stride))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    DeviceGuard g(device);
    return launch_sense(tel, cfg, state, hip_stream);
}

int32_t pp_sense_frame_host(const pp_scene_batch* tel, const pp_sensor_cfg* cfg, pp_sensor* state) {
    if (!sense_frame_ok(tel) || !sensor_ok(cfg, state, tel->car_stride)) return PP_ERR_ARG;
    const ppsensor::Truth T = truth_view(tel);
    for (int64_t s = 0; s < T.S; s++) ppsensor::sense_scene(T, s, *cfg, *state);
    return PP_OK;
}

// (a lone scfg or a lone sstate asks for the sensor and is refused; neither: none)
int32_t pp_rollout_sensed(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                          const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                          void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate, const pp_follow_cfg* fcfg,
                          pp_follow* fstate, const pp_lane_change_cfg* lcfg, pp_lane_change* lstate,
                          const pp_sensor_cfg* scfg, pp_sensor* sstate) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream,
                        Stages{kFollow, jstate ? jcfg : nullptr, jstate, fcfg, fstate, lcfg, lstate, scfg, sstate});
}

void pp_tracker_cfg_default(pp_tracker_cfg* c) { if (c) pptracker::cfg_default(c); }

int32_t pp_track_frame(const pp_scene_batch* seen, const pp_tracker_cfg* cfg, int32_t consume, pp_tracker* state,
                       int32_t device, void* hip_stream) {
    if (device < 0 || device >= kMaxDev || consume < 1 || !sense_frame_ok(seen) ||
        !tracker_ok(cfg, state, seen->car_stride))
        return PP_ERR_ARG;
    if (seen->n_scenes == 0) return PP_OK;
    DeviceGuard g(device);
    return launch_track(seen, cfg, consume, state, hip_stream);
}

int32_t pp_track_frame_host(const pp_scene_batch* seen, const pp_tracker_cfg* cfg, int32_t consume,
                            pp_tracker* state) {
    if (consume < 1 || !sense_frame_ok(seen) || !tracker_ok(cfg, state, seen->car_stride)) return PP_ERR_ARG;
    const ppsensor::Truth Z = truth_view(seen);
    for (int64_t s = 0; s < Z.S; s++) pptracker::track_scene(Z, s, *cfg, consume * 0.02, *state);
    return PP_OK;
}

// (a lone tcfg or a lone tstate asks for the tracker and is refused; neither: none)
int32_t pp_rollout_tracked(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                           const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                           void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate, const pp_follow_cfg* fcfg,
                           pp_follow* fstate, const pp_lane_change_cfg* lcfg, pp_lane_change* lstate,
                           const pp_sensor_cfg* scfg, pp_sensor* sstate, const pp_tracker_cfg* tcfg,
                           pp_tracker* tstate) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream,
                        Stages{kFollow, jstate ? jcfg : nullptr, jstate, fcfg, fstate, lcfg, lstate, scfg, sstate, tcfg,
                               tstate});
}

void pp_episode_cfg_default(pp_episode_cfg* c) { if (c) ppepisode::cfg_default(c); }

int32_t pp_synth_episode(pp_map* M, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                         const pp_follow_cfg* gap_rule, pp_scene_batch* tel, pp_traffic* traffic, pp_judge* jstate,
                         pp_follow* fstate, int32_t device, void* hip_stream) {
    pp_follow_cfg gap;
    if (device < 0 || device >= kMaxDev || !episode_ok(M, first_scene, cfg, gap_rule, tel, traffic, jstate, fstate, &gap))
        return PP_ERR_ARG;
    traffic->n_cars = cfg->n_cars;
    if (tel->n_scenes == 0) return PP_OK;
    const WorldDev W(M, device, false);
    if (W.rc) return W.rc;
    const ppsynth::OutBatch o = out_batch(tel);
    return launch_scenes(k_synth_episode, o.S, hip_stream, W.T, seed, first_scene, *cfg, gap, o, tel->tab_valid,
                         tel->tab_id, (int)tel->tab_slots, traffic_view(traffic, o.S), or_zero(jstate),
                         jstate ? 1 : 0, or_zero(fstate), fstate ? 1 : 0);
}

int32_t pp_synth_episode_host(const pp_map* M, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                              const pp_follow_cfg* gap_rule, pp_scene_batch* tel, pp_traffic* traffic,
                              pp_judge* jstate, pp_follow* fstate) {
    pp_follow_cfg gap;
    if (!episode_ok(M, first_scene, cfg, gap_rule, tel, traffic, jstate, fstate, &gap)) return PP_ERR_ARG;
    traffic->n_cars = cfg->n_cars;
    const WorldTables W = host_tables(M);
    const ppsynth::OutBatch o = out_batch(tel);
    const ppsynth::TrafficV tv = traffic_view(traffic, o.S);
    const pp_judge js = or_zero(jstate);
    const pp_follow fs = or_zero(fstate);
    for (int64_t s = 0; s < o.S; s++)
        ppepisode::episode_scene(W.T, seed, first_scene + s, s, *cfg, gap, o, tel->tab_valid, tel->tab_id,
                                 (int)tel->tab_slots, tv, js, jstate != nullptr, fs, fstate != nullptr);
    return PP_OK;
}

int32_t pp_judge_summary(pp_map* M, const pp_judge* state, int64_t n_scenes, const pp_summary_cfg* cfg,
                         pp_judge_stats* stats, int32_t device, void* hip_stream) {
    SumArgs A;
    if (!M || device < 0 || device >= kMaxDev || !summary_ok(state, n_scenes, cfg, stats) ||
        !summary_args(n_scenes, *cfg, A))
        return PP_ERR_ARG;
    if (n_scenes == 0) return PP_OK;
    return launch_summary(M, state, A, stats, device, hip_stream);
}

int32_t pp_judge_summary_host(const pp_judge* state, int64_t n_scenes, const pp_summary_cfg* cfg,
                              pp_judge_stats* stats) {
    if (!summary_ok(state, n_scenes, cfg, stats)) return PP_ERR_ARG;
    ppsummary::summarize_host(*state, n_scenes, *cfg, *stats);
    return PP_OK;
}

}  // extern "C"

namespace {
// Every set is checked against every call of its round before the first launch; the rounds are then
// the public entry points themselves, so a set's rows are what those calls made by hand produce.
// sensors: a sensor per set and its state (pp_rollout_sweep_sensed), or both null (pp_rollout_sweep);
// trackers: the same for the tracker (pp_rollout_sweep_tracked).
int32_t sweep_impl(pp_map* M, const pp_params* sets, const pp_sweep_cfg* cfg, const pp_episode_cfg* ecfg,
                   const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg, const pp_lane_change_cfg* lcfg,
                   pp_scene_batch* tel, pp_traffic* traffic, pp_result* res, pp_judge* jstate,
                   pp_follow* fstate, pp_lane_change* lstate, pp_judge_stats* stats, int32_t device,
                   void* hip_stream, const pp_sensor_cfg* sensors, pp_sensor* sstate,
                   const pp_tracker_cfg* trackers = nullptr, pp_tracker* tstate = nullptr) {
    pp_follow_cfg gap;
    if (!sets || !cfg || cfg->n_sets < 1 || !jstate || !fstate || device < 0 || device >= kMaxDev ||
        !episode_ok(M, cfg->first_scene, ecfg, fcfg, tel, traffic, jstate, fstate, &gap))
        return PP_ERR_ARG;
    const int64_t S = tel->n_scenes;
    pp_traffic placed = *traffic;                       // as pp_synth_episode leaves it
    placed.n_cars = ecfg->n_cars;
    for (int p = 0; p < cfg->n_sets; p++) {
        const Stages st{kFollow, jcfg, jstate, fcfg, fstate, lcfg, lstate, sensors ? &sensors[p] : nullptr, sstate,
                        trackers ? &trackers[p] : nullptr, tstate};
        if (!rollout_ok(M, tel, &placed, &sets[p], &cfg->rollout, res, nullptr, device, st) ||
            eval_check(M, tel, &sets[p], res, device) != PP_OK)
            return PP_ERR_ARG;
    }
    pp_summary_cfg sc = cfg->summary;
    if (sc.scenes_per_group < 1) return PP_ERR_ARG;
    const int64_t G = ppsummary::n_groups(S, sc.scenes_per_group);
    sc.out_first = 0;
    sc.out_stride = cfg->n_sets * G;
    SumArgs A;
    if (!summary_ok(jstate, S, &sc, stats) || !summary_args(S, sc, A)) return PP_ERR_ARG;
    if (S == 0) return PP_OK;
    for (int p = 0; p < cfg->n_sets; p++) {
        int rc = pp_synth_episode(M, cfg->seed, cfg->first_scene, ecfg, fcfg, tel, traffic, jstate, fstate, device,
                                  hip_stream);
        if (rc == PP_OK && lstate) {
            DeviceGuard g(device);
            if (hipMemsetAsync(lstate->started, 0, sizeof(int32_t) * (size_t)S, (hipStream_t)hip_stream) != hipSuccess)
                rc = PP_ERR_HIP;
        }
        if (rc == PP_OK && sstate) {
            DeviceGuard g(device);
            if (hipMemsetAsync(sstate->frame, 0, sizeof(int32_t) * (size_t)S, (hipStream_t)hip_stream) != hipSuccess)
                rc = PP_ERR_HIP;
        }
        if (rc == PP_OK && tstate) {
            DeviceGuard g(device);
            if (hipMemsetAsync(tstate->frame, 0, sizeof(int32_t) * (size_t)S, (hipStream_t)hip_stream) != hipSuccess)
                rc = PP_ERR_HIP;
        }
        if (rc == PP_OK)
            rc = pp_rollout_tracked(M, tel, traffic, &sets[p], &cfg->rollout, res, nullptr, device, hip_stream, jcfg,
                                    jstate, fcfg, fstate, lcfg, lstate, sensors ? &sensors[p] : nullptr, sstate,
                                    trackers ? &trackers[p] : nullptr, tstate);
        sc.out_first = p * G;
        if (rc == PP_OK) rc = pp_judge_summary(M, jstate, S, &sc, stats, device, hip_stream);
        if (rc != PP_OK) return rc;
    }
    return PP_OK;
}
}  // namespace

extern "C" {

int32_t pp_rollout_sweep(pp_map* M, const pp_params* sets, const pp_sweep_cfg* cfg, const pp_episode_cfg* ecfg,
                         const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg, const pp_lane_change_cfg* lcfg,
                         pp_scene_batch* tel, pp_traffic* traffic, pp_result* res, pp_judge* jstate,
                         pp_follow* fstate, pp_lane_change* lstate, pp_judge_stats* stats, int32_t device,
                         void* hip_stream) {
    return sweep_impl(M, sets, cfg, ecfg, jcfg, fcfg, lcfg, tel, traffic, res, jstate, fstate, lstate, stats, device,
                      hip_stream, nullptr, nullptr);
}

int32_t pp_rollout_sweep_sensed(pp_map* M, const pp_params* sets, const pp_sweep_cfg* cfg, const pp_episode_cfg* ecfg,
                                const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg, const pp_lane_change_cfg* lcfg,
                                pp_scene_batch* tel, pp_traffic* traffic, pp_result* res, pp_judge* jstate,
                                pp_follow* fstate, pp_lane_change* lstate, pp_judge_stats* stats, int32_t device,
                                void* hip_stream, const pp_sensor_cfg* sensor_sets, pp_sensor* sstate) {
    if (!sensor_sets || !sstate) return PP_ERR_ARG;
    return sweep_impl(M, sets, cfg, ecfg, jcfg, fcfg, lcfg, tel, traffic, res, jstate, fstate, lstate, stats, device,
                      hip_stream, sensor_sets, sstate);
}

int32_t pp_rollout_sweep_tracked(pp_map* M, const pp_params* sets, const pp_sweep_cfg* cfg, const pp_episode_cfg* ecfg,
                                 const pp_judge_cfg* jcfg, const pp_follow_cfg* fcfg, const pp_lane_change_cfg* lcfg,
                                 pp_scene_batch* tel, pp_traffic* traffic, pp_result* res, pp_judge* jstate,
                                 pp_follow* fstate, pp_lane_change* lstate, pp_judge_stats* stats, int32_t device,
                                 void* hip_stream, const pp_sensor_cfg* sensor_sets, pp_sensor* sstate,
                                 const pp_tracker_cfg* tracker_sets, pp_tracker* tstate) {
    if (!sensor_sets || !sstate || !tracker_sets || !tstate) return PP_ERR_ARG;
    return sweep_impl(M, sets, cfg, ecfg, jcfg, fcfg, lcfg, tel, traffic, res, jstate, fstate, lstate, stats, device,
                      hip_stream, sensor_sets, sstate, tracker_sets, tstate);
}

}  // extern "C"
