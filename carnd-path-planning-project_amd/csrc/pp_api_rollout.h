// pp_api_rollout.h — host: closed-loop rollouts, the judge and reactive traffic (C ABI).
// Part of pp_eval.hip's translation unit.
#pragma once

namespace {
void launch_judge(const ppsynth::LaneTables& T, const pp_scene_batch* tel, const ppsynth::TrafficV& tv,
                  const pp_result* plan, int32_t consume, const pp_judge_cfg* jc, const pp_judge* js,
                  hipStream_t stream) {
    const int64_t S = tel->n_scenes;
    hipLaunchKernelGGL(k_judge, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, T, S, tel->ego_x,
                       tel->ego_y, tel->ego_yaw_deg, plan->next_x, plan->next_y, plan->n_out, tv, consume, *jc, *js);
}

void launch_follow(const ppsynth::LaneTables& T, const ppfollow::ArcTables& AT, const pp_scene_batch* tel,
                   const ppsynth::TrafficV& tv, int32_t consume, const pp_follow_cfg* fc, const pp_follow* fs,
                   hipStream_t stream) {
    const int64_t S = tel->n_scenes;
    hipLaunchKernelGGL(k_follow, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, T, AT, S, tel->ego_x,
                       tel->ego_y, tel->ego_speed_mph, tv, consume, *fc, *fs);
}

void launch_lane_change(const ppsynth::LaneTables& T, const ppfollow::ArcTables& AT, const pp_scene_batch* tel,
                        const ppsynth::TrafficV& tv, int32_t consume, const pp_follow_cfg* fc, const pp_follow* fs,
                        const pp_lane_change_cfg* lc, const pp_lane_change* ls, hipStream_t stream) {
    const int64_t S = tel->n_scenes;
    hipLaunchKernelGGL(k_lane_change, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, T, AT, S, tel->ego_x,
                       tel->ego_y, tel->ego_speed_mph, tv, consume, *fc, *fs, *lc, *ls);
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
    if (js && (!js->steps || !js->flags || !js->count || !js->first_step || !js->first_car || !js->seg_hint ||
               !js->off_run || !js->head_x || !js->head_y || !js->ring_vx || !js->ring_vy || !js->dist ||
               !js->clean_dist || !js->min_sep || !js->max_speed_mph || !js->max_acc || !js->max_jerk))
        return false;
    if (fs && (!fs->started || !fs->ego_seg || !fs->desired || !fs->next_speed || !fs->leader || !fs->gap)) return false;
    if (!ppepisode::cfg_ok(*cfg) || cfg->n_cars > tel->car_stride) return false;
    if (tel->tab_valid && (tel->tab_slots < cfg->n_cars || tel->tab_slots > PP_MAX_CARS)) return false;
    if (gap_rule) *gap = *gap_rule; else pp_follow_cfg_default(gap);
    // (the follow update takes any headway and standstill gap; a placement by them needs numbers >= 0)
    if (!ppfollow::cfg_ok(*gap) || !(gap->time_headway >= 0) || !(gap->min_gap >= 0)) return false;
    const ppfollow::ArcTables A = ppfollow::arc_tables(M->arctab.data(), M->n);
    double min_loop = A.loop[0];
    for (int l = 1; l < PP_NUM_LANES; l++) min_loop = A.loop[l] < min_loop ? A.loop[l] : min_loop;
    return ppepisode::ring_ok(*cfg, *gap, min_loop);
}

// pp_rollout's loop; with follow state (fc, fs non-null) k_follow runs after pp_eval, with lane-change
// state (lc, ls non-null; needs the follow state) k_lane_change after k_follow, with a judge (jc, js
// non-null) k_judge runs before k_sim
int32_t rollout_loop(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                     const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                     void* hip_stream, const pp_judge_cfg* jc, const pp_judge* js,
                     const pp_follow_cfg* fc = nullptr, const pp_follow* fs = nullptr,
                     const pp_lane_change_cfg* lc = nullptr, const pp_lane_change* ls = nullptr) {
    if (!M || !tel || !prm || !cfg || !res || device < 0 || device >= kMaxDev || !traffic_ok(traffic, tel))
        return PP_ERR_ARG;
    if (cfg->n_frames < 0 || cfg->consume < 1 || !(cfg->sensor_range >= 0) || prm->n_draws > 1 ||
        prm->emit_paths || !tel->tab_valid || !tel->tab_lane || !tel->tab_s || !tel->tab_d ||
        !tel->tab_vs || !tel->tab_vd || !tel->tab_vx || !tel->tab_vy || tel->car_stride < traffic->n_cars ||
        tel->tab_slots < traffic->n_cars)
        return PP_ERR_ARG;
    if (log && log->plan_x && !log->plan_y) return PP_ERR_ARG;
    if (tel->n_scenes == 0 || cfg->n_frames == 0) return PP_OK;
    DeviceGuard g(device);
    ppsynth::LaneTables T;
    ppfollow::ArcTables AT = {nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(M->mu);
        const int rc = dev_init(M, device);
        if (rc) return rc;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
        if (fs) {
            const int ra = arc_init(M, device);
            if (ra) return ra;
            AT = ppfollow::arc_tables(M->dev[device].arctab.get(), M->n);
        }
    }
    SimArgs A;
    A.consume = cfg->consume;
    A.range2 = cfg->sensor_range * cfg->sensor_range;
    if (log) A.log = *log; else memset(&A.log, 0, sizeof(A.log));
    const ppsynth::TrafficV tv = traffic_view(traffic, tel->n_scenes);
    const int64_t blocks = (tel->n_scenes + 255) / 256;
    for (int f = 0; f < cfg->n_frames; f++) {
        const int rc = pp_eval(M, tel, prm, res, device, hip_stream);
        if (rc != PP_OK) return rc;
        if (fs) {
            launch_follow(T, AT, tel, tv, cfg->consume, fc, fs, (hipStream_t)hip_stream);
            if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
        }
        if (ls && tv.n > 0) {
            launch_lane_change(T, AT, tel, tv, cfg->consume, fc, fs, lc, ls, (hipStream_t)hip_stream);
            if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
        }
        if (js) {
            launch_judge(T, tel, tv, res, cfg->consume, jc, js, (hipStream_t)hip_stream);
            if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
        }
        A.frame = f;
        hipLaunchKernelGGL(k_sim, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, T, *tel,
                           tv, *prm, *res, A);
        if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    }
    return PP_OK;
}
}  // namespace

extern "C" {

int32_t pp_rollout(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                   const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                   void* hip_stream) {
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, nullptr, nullptr);
}

int32_t pp_rollout_judged(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                          const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                          void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* state) {
    if (!judge_ok(jcfg, state) || !cfg || !judge_frame_ok(tel, traffic, res, cfg->consume)) return PP_ERR_ARG;
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, jcfg, state);
}

void pp_judge_cfg_default(pp_judge_cfg* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->speed_limit_mph = 50;
    c->max_acc = 10;
    c->max_jerk = 10;
    c->ego_length = c->car_length = 4.5;
    c->ego_width = c->car_width = 2.0;
    c->lane_tol = 1.0;
    c->acc_window = 10;
    c->jerk_window = 50;
    c->off_lane_steps = 150;
}

int32_t pp_judge_frame(pp_map* M, const pp_scene_batch* tel, const pp_traffic* traffic, const pp_result* plan,
                       int32_t consume, const pp_judge_cfg* cfg, pp_judge* state, int32_t device,
                       void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !judge_ok(cfg, state) ||
        !judge_frame_ok(tel, traffic, plan, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    DeviceGuard g(device);
    ppsynth::LaneTables T;
    {
        std::lock_guard<std::mutex> lk(M->mu);
        const int rc = dev_init(M, device);
        if (rc) return rc;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
    }
    launch_judge(T, tel, traffic_view(traffic, tel->n_scenes), plan, consume, cfg, state, (hipStream_t)hip_stream);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

int32_t pp_judge_frame_host(const pp_map* M, const pp_scene_batch* tel, const pp_traffic* traffic,
                            const pp_result* plan, int32_t consume, const pp_judge_cfg* cfg, pp_judge* state) {
    if (!M || !judge_ok(cfg, state) || !judge_frame_ok(tel, traffic, plan, consume)) return PP_ERR_ARG;
    const ppsynth::LaneTables T = lane_tables(M->lanetab.data(), M->n);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        ppjudge::judge_scene(T, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_yaw_deg[s], plan->next_x, plan->next_y,
                             plan->n_out[s], tv, consume, *cfg, *state);
    return PP_OK;
}

int32_t pp_rollout_reactive(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                            const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                            void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate,
                            const pp_follow_cfg* fcfg, pp_follow* fstate) {
    if (!follow_ok(fcfg, fstate) || !cfg || !follow_frame_ok(tel, traffic, cfg->consume)) return PP_ERR_ARG;
    if (jstate && (!judge_ok(jcfg, jstate) || !judge_frame_ok(tel, traffic, res, cfg->consume))) return PP_ERR_ARG;
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, jstate ? jcfg : nullptr, jstate,
                        fcfg, fstate);
}

void pp_follow_cfg_default(pp_follow_cfg* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_acc = 2.0;
    c->comfort_brake = 3.0;
    c->max_brake = 8.0;
    c->time_headway = 1.2;
    c->min_gap = 2.0;
    c->gap_floor = 0.5;
    c->horizon = 150;
    c->car_length = c->ego_length = 4.5;
    c->lateral_reach = 2.0;
    c->react_to_ego = 1;
}

int32_t pp_traffic_follow(pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                          const pp_follow_cfg* cfg, pp_follow* state, int32_t device, void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !follow_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    DeviceGuard g(device);
    ppsynth::LaneTables T;
    ppfollow::ArcTables AT;
    {
        std::lock_guard<std::mutex> lk(M->mu);
        int rc = dev_init(M, device);
        if (rc) return rc;
        rc = arc_init(M, device);
        if (rc) return rc;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
        AT = ppfollow::arc_tables(M->dev[device].arctab.get(), M->n);
    }
    launch_follow(T, AT, tel, traffic_view(traffic, tel->n_scenes), consume, cfg, state, (hipStream_t)hip_stream);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

void pp_lane_change_cfg_default(pp_lane_change_cfg* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->politeness = 0.3;
    c->threshold = 0.2;
    c->right_bias = 0.0;
    c->safe_brake = 3.0;
    c->lateral_speed = 1.5;
    c->ego_desired_speed = 22.2;
    c->min_interval_steps = 250;
}

int32_t pp_traffic_lane_change(pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                               const pp_follow_cfg* fcfg, const pp_follow* fstate, const pp_lane_change_cfg* cfg,
                               pp_lane_change* state, int32_t device, void* hip_stream) {
    if (!M || device < 0 || device >= kMaxDev || !follow_ok(fcfg, fstate) || !lane_change_ok(cfg, state) ||
        !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0 || traffic->n_cars == 0) return PP_OK;
    DeviceGuard g(device);
    ppsynth::LaneTables T;
    ppfollow::ArcTables AT;
    {
        std::lock_guard<std::mutex> lk(M->mu);
        int rc = dev_init(M, device);
        if (rc) return rc;
        rc = arc_init(M, device);
        if (rc) return rc;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
        AT = ppfollow::arc_tables(M->dev[device].arctab.get(), M->n);
    }
    launch_lane_change(T, AT, tel, traffic_view(traffic, tel->n_scenes), consume, fcfg, fstate, cfg, state,
                       (hipStream_t)hip_stream);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

int32_t pp_traffic_lane_change_host(const pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                                    const pp_follow_cfg* fcfg, const pp_follow* fstate,
                                    const pp_lane_change_cfg* cfg, pp_lane_change* state) {
    if (!M || !follow_ok(fcfg, fstate) || !lane_change_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume))
        return PP_ERR_ARG;
    if (traffic->n_cars == 0) return PP_OK;
    const ppsynth::LaneTables T = lane_tables(M->lanetab.data(), M->n);
    const ppfollow::ArcTables AT = ppfollow::arc_tables(M->arctab.data(), M->n);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        pplanechange::lane_change_scene(T, AT, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_speed_mph[s], tv, consume,
                                        *fcfg, *fstate, *cfg, *state);
    return PP_OK;
}

int32_t pp_rollout_lane_changing(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                                 const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                                 void* hip_stream, const pp_judge_cfg* jcfg, pp_judge* jstate,
                                 const pp_follow_cfg* fcfg, pp_follow* fstate, const pp_lane_change_cfg* lcfg,
                                 pp_lane_change* lstate) {
    if (!follow_ok(fcfg, fstate) || !cfg || !follow_frame_ok(tel, traffic, cfg->consume)) return PP_ERR_ARG;
    if (jstate && (!judge_ok(jcfg, jstate) || !judge_frame_ok(tel, traffic, res, cfg->consume))) return PP_ERR_ARG;
    if ((lcfg || lstate) && !lane_change_ok(lcfg, lstate)) return PP_ERR_ARG;
    return rollout_loop(M, tel, traffic, prm, cfg, res, log, device, hip_stream, jstate ? jcfg : nullptr, jstate,
                        fcfg, fstate, lstate ? lcfg : nullptr, lstate);
}

void pp_episode_cfg_default(pp_episode_cfg* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->n_cars = 12;
    c->ego_speed_min = 0;
    c->ego_speed_max = 20;
    c->car_speed_min = 5;
    c->car_speed_max = 25;
    c->ahead_share = 0.75;
    c->extra_gap = 40;
    c->offset_jitter = 0.3;
    c->gap_slack = 1e-6;
}

int32_t pp_synth_episode(pp_map* M, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                         const pp_follow_cfg* gap_rule, pp_scene_batch* tel, pp_traffic* traffic, pp_judge* jstate,
                         pp_follow* fstate, int32_t device, void* hip_stream) {
    pp_follow_cfg gap;
    if (device < 0 || device >= kMaxDev || !episode_ok(M, first_scene, cfg, gap_rule, tel, traffic, jstate, fstate, &gap))
        return PP_ERR_ARG;
    traffic->n_cars = cfg->n_cars;
    if (tel->n_scenes == 0) return PP_OK;
    DeviceGuard g(device);
    ppsynth::LaneTables T;
    {
        std::lock_guard<std::mutex> lk(M->mu);
        const int rc = dev_init(M, device);
        if (rc) return rc;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
    }
    const ppsynth::OutBatch o = out_batch(tel);
    pp_judge js;
    pp_follow fs;
    memset(&js, 0, sizeof(js));
    memset(&fs, 0, sizeof(fs));
    if (jstate) js = *jstate;
    if (fstate) fs = *fstate;
    hipLaunchKernelGGL(k_synth_episode, dim3((unsigned)((o.S + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, T,
                       seed, first_scene, *cfg, gap, o, tel->tab_valid, tel->tab_id, (int)tel->tab_slots,
                       traffic_view(traffic, o.S), js, jstate ? 1 : 0, fs, fstate ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

int32_t pp_synth_episode_host(const pp_map* M, uint64_t seed, int64_t first_scene, const pp_episode_cfg* cfg,
                              const pp_follow_cfg* gap_rule, pp_scene_batch* tel, pp_traffic* traffic,
                              pp_judge* jstate, pp_follow* fstate) {
    pp_follow_cfg gap;
    if (!episode_ok(M, first_scene, cfg, gap_rule, tel, traffic, jstate, fstate, &gap)) return PP_ERR_ARG;
    traffic->n_cars = cfg->n_cars;
    const ppsynth::LaneTables T = lane_tables(M->lanetab.data(), M->n);
    const ppsynth::OutBatch o = out_batch(tel);
    const ppsynth::TrafficV tv = traffic_view(traffic, o.S);
    pp_judge js;
    pp_follow fs;
    memset(&js, 0, sizeof(js));
    memset(&fs, 0, sizeof(fs));
    if (jstate) js = *jstate;
    if (fstate) fs = *fstate;
    for (int64_t s = 0; s < o.S; s++)
        ppepisode::episode_scene(T, seed, first_scene + s, s, *cfg, gap, o, tel->tab_valid, tel->tab_id,
                                 (int)tel->tab_slots, tv, js, jstate != nullptr, fs, fstate != nullptr);
    return PP_OK;
}

int32_t pp_traffic_follow_host(const pp_map* M, const pp_scene_batch* tel, pp_traffic* traffic, int32_t consume,
                               const pp_follow_cfg* cfg, pp_follow* state) {
    if (!M || !follow_ok(cfg, state) || !follow_frame_ok(tel, traffic, consume)) return PP_ERR_ARG;
    const ppsynth::LaneTables T = lane_tables(M->lanetab.data(), M->n);
    const ppfollow::ArcTables AT = ppfollow::arc_tables(M->arctab.data(), M->n);
    const int64_t S = tel->n_scenes;
    const ppsynth::TrafficV tv = traffic_view(traffic, S);
    for (int64_t s = 0; s < S; s++)
        ppfollow::follow_scene(T, AT, S, s, tel->ego_x[s], tel->ego_y[s], tel->ego_speed_mph[s], tv, consume, *cfg,
                               *state);
    return PP_OK;
}

}  // extern "C"
