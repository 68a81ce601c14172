// pp_episode.h — drivable episode starts (include/pp.h pp_synth_episode; DESIGN.md "Episode starts").
//
// One function writes the start state of one scene for a judged, reactive drive: the ego on a lane
// centre with its previous path AHEAD of it, traffic placed car by car at no less than the gap the
// car-following model asks for (csrc/pp_follow.h's s*), the frame-0 telemetry of that traffic, a WARM
// judge state (the velocity ring filled with the start velocity, so no start transient is recorded)
// and a zeroed follow state. The definitions are this project's own. Compiled for the device
// (k_synth_episode) and the host (pp_synth_episode_host): only + - * / sqrt on the same inputs in
// the same order under -ffp-contract=off, plus ppg::atan2 for the yaw, so the two agree bit for bit.
//
// Random numbers: one ppsynth::Rng stream per scene, key = seed, counter = (global scene index,
// block, kTag). kTag differs from pp_synth_scenes' counter word, so the two generators draw
// unrelated values from one seed. The draw order is fixed:
//   ego:      seg = below(n), t = uni(), lane = below(PP_NUM_LANES), ve = uni(ego_speed_min, ego_speed_max)
//   car j:    lane = below(PP_NUM_LANES), v = uni(car_speed_min, car_speed_max), side = uni(),
//             extra = uni(0, extra_gap), offset = uni(-offset_jitter, offset_jitter)
// for j = 0 .. n_cars - 1 in order; every draw is made whatever the configuration's values, so a scene
// depends only on (seed, global index, cfg) and shards concatenate.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "../../include/pp.h"
#include "pp_synth.h"
#include "pp_follow.h"

namespace ppepisode {

constexpr uint32_t kTag = 0xE9150DE1u;     // the stream's fourth counter word

// pp_episode_cfg_default's values (host only)
inline void cfg_default(pp_episode_cfg* c) {
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

// true also rejects NaN: every comparison is written so that a NaN fails it
PP_HD inline bool cfg_ok(const pp_episode_cfg& c) {
    return c.n_cars >= 0 && c.n_cars <= PP_MAX_CARS && c.ego_speed_min >= 0 && c.ego_speed_max >= c.ego_speed_min &&
           c.car_speed_min >= 0 && c.car_speed_max >= c.car_speed_min && c.ahead_share >= 0 && c.ahead_share <= 1 &&
           c.extra_gap >= 0 && c.offset_jitter >= 0 && c.gap_slack >= 0 && c.ego_speed_max < INFINITY &&
           c.car_speed_max < INFINITY && c.extra_gap < INFINITY && c.offset_jitter < INFINITY &&
           c.gap_slack < INFINITY;
}

// The net gap a follower at vf needs behind a leader at vl: follow_scene's sstar, the same operations.
PP_HD inline double req(const pp_follow_cfg& g, double two_sab, double vf, double vl) {
    const double dyn = vf * g.time_headway + vf * (vf - vl) / two_sab;
    return g.min_gap + (dyn > 0 ? dyn : 0.0);
}

// The ring is long enough: the front and back cursors of a lane cannot meet round the loop even when
// every car takes the largest step. min_loop: the shortest lane's ring (ArcTables::loop).
PP_HD inline bool ring_ok(const pp_episode_cfg& c, const pp_follow_cfg& g, double min_loop) {
    const double vmax = c.ego_speed_max > c.car_speed_max ? c.ego_speed_max : c.car_speed_max;
    const double vmin = c.ego_speed_min < c.car_speed_min ? c.ego_speed_min : c.car_speed_min;
    const double mixed = (g.car_length + g.ego_length) / 2;
    const double len = g.car_length > mixed ? g.car_length : mixed;
    const double step = req(g, 2 * sqrt(g.max_acc * g.comfort_brake), vmax, vmin) + c.gap_slack + c.extra_gap + len;
    return (c.n_cars + 1) * step <= min_loop;        // (false for a NaN step)
}

// Writes scene `s` of the batch from global index `g` (all arrays [k * S + s]). o: the telemetry;
// tab_valid/tab_id/tab_slots: its car table (tab_valid may be null); tr: the traffic (tr.n =
// cfg.n_cars); js, fs: the judge and follow states, written only when has_js, has_fs (by reference
// and flag, not by pointer: the address of a kernel argument would put it in scratch).
PP_HD inline void episode_scene(const ppsynth::LaneTables& T, uint64_t seed, int64_t g, int64_t s,
                                const pp_episode_cfg& cfg, const pp_follow_cfg& gap,
                                const ppsynth::OutBatch& o, int32_t* tab_valid, int32_t* tab_id, int tab_slots,
                                const ppsynth::TrafficV& tr, const pp_judge& js, bool has_js, const pp_follow& fs,
                                bool has_fs) {
    ppsynth::Rng r(seed, (uint64_t)g, kTag);
    const int64_t S = o.S;
    const int n = T.n;

    // ego: on the lane centre, heading along the segment
    const int seg = r.below(n);
    const double t = r.uni();
    const int lane = r.below(PP_NUM_LANES);
    const double ve = r.uni(cfg.ego_speed_min, cfg.ego_speed_max);
    const int ip = (seg == 0) ? n - 1 : seg - 1;
    const double ax = T.lc_x[lane * n + ip], ay = T.lc_y[lane * n + ip];
    const double bx = T.lc_x[lane * n + seg], by = T.lc_y[lane * n + seg];
    const double px = ax + (bx - ax) * t, py = ay + (by - ay) * t;
    const double ux = T.tan_x[lane * n + seg], uy = T.tan_y[lane * n + seg];
    o.ego_x[s] = px;
    o.ego_y[s] = py;
    o.ego_yaw_deg[s] = ppg::atan2(uy, ux) * 180.0 / 3.14159265358979323846;   // glibc's, host == device
    o.ego_speed_mph[s] = ve * 2.237;
    o.prev_target_lane[s] = lane;
    // previous path: ahead of the ego on the straight line along u, one driven step apart
    const double step = ve * 0.02;
    for (int k = 0; k < PP_PREV_KEEP; k++) {
        const double d = (k + 1) * step;
        o.prev_x[(int64_t)k * S + s] = px + d * ux;
        o.prev_y[(int64_t)k * S + s] = py + d * uy;
    }
    o.n_prev[s] = ve > 0 ? PP_PREV_KEEP : 0;

    // cars: per lane a front and a back cursor (arc relative to the ego's (seg, t), speed), both
    // starting at the ego. PP_NUM_LANES-element arrays touched only in fully unrolled select loops
    // (registers); moved_f/moved_b: bit l set once lane l's cursor is a car and no longer the ego.
    double a_f[PP_NUM_LANES], v_f[PP_NUM_LANES], a_b[PP_NUM_LANES], v_b[PP_NUM_LANES];
#pragma unroll
    for (int l = 0; l < PP_NUM_LANES; l++) { a_f[l] = 0.0; v_f[l] = ve; a_b[l] = 0.0; v_b[l] = ve; }
    uint32_t moved_f = 0, moved_b = 0;
    const double two_sab = 2 * sqrt(gap.max_acc * gap.comfort_brake);
    const double len_ego = (gap.car_length + gap.ego_length) / 2;
    const int J = cfg.n_cars;
    o.n_cars[s] = J;
    for (int j = 0; j < J; j++) {
        const int cl = r.below(PP_NUM_LANES);
        const double v = r.uni(cfg.car_speed_min, cfg.car_speed_max);
        const bool ahead = r.uni() < cfg.ahead_share;
        const double extra = r.uni(0.0, cfg.extra_gap);
        const double off = r.uni(-cfg.offset_jitter, cfg.offset_jitter);
        double af = 0, vf = 0, ab = 0, vb = 0;
#pragma unroll
        for (int l = 0; l < PP_NUM_LANES; l++)
            if (cl == l) { af = a_f[l]; vf = v_f[l]; ab = a_b[l]; vb = v_b[l]; }
        const uint32_t bit = 1u << cl;
        double ds;
        if (ahead) {
            const double len = (moved_f & bit) ? gap.car_length : len_ego;
            ds = af + req(gap, two_sab, vf, v) + cfg.gap_slack + extra + len;
            moved_f |= bit;
        } else {
            const double len = (moved_b & bit) ? gap.car_length : len_ego;
            ds = ab - (req(gap, two_sab, v, vb) + cfg.gap_slack + extra + len);
            moved_b |= bit;
        }
#pragma unroll
        for (int l = 0; l < PP_NUM_LANES; l++)
            if (cl == l) {
                if (ahead) { a_f[l] = ds; v_f[l] = v; } else { a_b[l] = ds; v_b[l] = v; }
            }
        double qx, qy, qux, quy, ct;
        int cseg;
        ppsynth::lane_walk(T, cl, seg, t, ds, &qx, &qy, &qux, &quy, &cseg, &ct);
        const int64_t tx = (int64_t)j * tr.S + s;
        tr.lane[tx] = cl; tr.seg[tx] = cseg; tr.t[tx] = ct; tr.off[tx] = off; tr.v[tx] = v;
        // frame-0 telemetry: every car is reported, as k_sim reports it
        const int64_t ix = (int64_t)j * S + s;
        double cx, cy, cvx, cvy;
        ppsynth::traffic_car(T, cl, cseg, ct, off, v, &cx, &cy, &cvx, &cvy);
        o.car_id[ix] = j;
        o.car_x[ix] = cx; o.car_y[ix] = cy; o.car_vx[ix] = cvx; o.car_vy[ix] = cvy;
    }
    for (int k = 0; tab_valid && k < tab_slots; k++) {               // empty table, slot k = car k
        tab_valid[(int64_t)k * S + s] = 0;
        if (tab_id) tab_id[(int64_t)k * S + s] = k;
    }

    if (has_js) {   // a carried state PP_JUDGE_RING steps into a drive at the start velocity
        const double vx = ve * ux, vy = ve * uy;
        js.steps[s] = PP_JUDGE_RING;
        js.flags[s] = 0;
        for (int k = 0; k < PP_INC_KINDS; k++) { js.count[(int64_t)k * S + s] = 0; js.first_step[(int64_t)k * S + s] = 0; }
        js.first_car[s] = 0; js.seg_hint[s] = seg; js.off_run[s] = 0;
        js.head_x[s] = ux; js.head_y[s] = uy;
        for (int k = 0; k < PP_JUDGE_RING; k++) { js.ring_vx[(int64_t)k * S + s] = vx; js.ring_vy[(int64_t)k * S + s] = vy; }
        js.dist[s] = 0.0; js.clean_dist[s] = 0.0; js.min_sep[s] = INFINITY;
        js.max_speed_mph[s] = 0.0; js.max_acc[s] = 0.0; js.max_jerk[s] = 0.0;
    }
    if (has_fs) { fs.started[s] = 0; fs.ego_seg[s] = 0; }
}

}  // namespace ppepisode
