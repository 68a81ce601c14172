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

// pp_rollout's loop; with follow state (fc, fs non-null) k_follow runs after pp_eval, with a judge (jc,
// js non-null) k_judge runs before k_sim
int32_t rollout_loop(pp_map* M, pp_scene_batch* tel, pp_traffic* traffic, const pp_params* prm,
                     const pp_rollout_cfg* cfg, pp_result* res, pp_rollout_log* log, int32_t device,
                     void* hip_stream, const pp_judge_cfg* jc, const pp_judge* js,
                     const pp_follow_cfg* fc = nullptr, const pp_follow* fs = nullptr) {
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
        T = lane_tables(M->dev[device].lanetab, M->n);
        if (fs) {
            const int ra = arc_init(M, device);
            if (ra) return ra;
            AT = ppfollow::arc_tables(M->dev[device].arctab, M->n);
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
        T = lane_tables(M->dev[device].lanetab, M->n);
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
        T = lane_tables(M->dev[device].lanetab, M->n);
        AT = ppfollow::arc_tables(M->dev[device].arctab, M->n);
    }
    launch_follow(T, AT, tel, traffic_view(traffic, tel->n_scenes), consume, cfg, state, (hipStream_t)hip_stream);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
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
