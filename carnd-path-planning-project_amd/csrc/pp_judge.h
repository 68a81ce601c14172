// pp_judge.h — the rollout judge (include/pp.h pp_judge_frame; DESIGN.md "Rollout judge").
//
// One function judges the driven steps of one frame of one scene: the ego's plan points against
// the speed, acceleration and jerk limits, the lane-centre polylines and the rectangles of every
// traffic car. The definitions are this project's own, modelled on the published rules of the
// simulator the reference planner was written for (which is not available: nothing here is
// compared with it). Compiled for the device (k_judge) and the host (pp_judge_frame_host): only
// + - * / sqrt and ppg::cos/sin on the same inputs in the same order, under -ffp-contract=off on
// both sides, so the two agree bit for bit.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "../../include/pp.h"
#include "pp_synth.h"

namespace ppjudge {

constexpr double kDt = 0.02;               // one driven step (the simulator's 50 Hz)
constexpr int kRingMask = PP_JUDGE_RING - 1;
static_assert((PP_JUDGE_RING & kRingMask) == 0, "PP_JUDGE_RING must be a power of two");

// pp_judge_cfg_default's values (host only)
inline void cfg_default(pp_judge_cfg* c) {
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

PP_HD inline bool cfg_ok(const pp_judge_cfg& c) {
    return c.acc_window >= 1 && c.jerk_window >= 1 && c.acc_window <= kRingMask &&
           c.jerk_window <= kRingMask && c.acc_window + c.jerk_window <= kRingMask;
}

PP_HD inline double abs_(double x) { return x < 0 ? -x : x; }

// Separation of two rectangles by the separating-axis test: the largest gap over the four axes
// (<= 0: they overlap). Ego: centre p, unit axis h, half extents (ehl, ehw); car: centre c, unit
// axis u, half extents (chl, chw). The second axis of each is (y, -x) of its first.
PP_HD inline double rect_sep(double px, double py, double hx, double hy, double ehl, double ehw,
                             double cx, double cy, double ux, double uy, double chl, double chw) {
    const double dx = cx - px, dy = cy - py;
    const double ax[4] = {hx, hy, ux, uy};
    const double ay[4] = {hy, -hx, uy, -ux};
    double sep = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double re = ehl * abs_(ax[k] * hx + ay[k] * hy) + ehw * abs_(ax[k] * hy + ay[k] * -hx);
        const double rc = chl * abs_(ax[k] * ux + ay[k] * uy) + chw * abs_(ax[k] * uy + ay[k] * -ux);
        const double gap = abs_(ax[k] * dx + ay[k] * dy) - re - rc;
        if (k == 0 || gap > sep) sep = gap;
    }
    return sep;
}

// Squared distance from p to segment `seg` (from waypoint seg-1 to waypoint seg) of lane `lane`.
PP_HD inline double seg_dist2(const ppsynth::LaneTables& T, int lane, int seg, double px, double py) {
    const int n = T.n;
    const int ip = (seg == 0) ? n - 1 : seg - 1;
    const double ax = T.lc_x[lane * n + ip], ay = T.lc_y[lane * n + ip];
    const double bx = T.lc_x[lane * n + seg], by = T.lc_y[lane * n + seg];
    const double ex = bx - ax, ey = by - ay;
    const double ee = ex * ex + ey * ey;
    double t = ee > 0 ? ((px - ax) * ex + (py - ay) * ey) / ee : 0.0;
    t = t < 0 ? 0.0 : (t > 1 ? 1.0 : t);
    const double qx = px - (ax + ex * t), qy = py - (ay + ey * t);
    return qx * qx + qy * qy;
}

// Judges driven steps 1..consume of scene s for one frame (all arrays [k * S + s]). (x0, y0),
// yaw_deg: the ego before the frame; next_x/next_y, n_out: the frame's plan; tr: the traffic
// before the frame (read only); st: the scene's carried state and accumulators (updated).
PP_HD inline void judge_scene(const ppsynth::LaneTables& T, int64_t S, int64_t s, double x0, double y0,
                              double yaw_deg, const double* next_x, const double* next_y, int n_out,
                              const ppsynth::TrafficV& tr, int consume, const pp_judge_cfg& cfg,
                              const pp_judge& st) {
    const int n_wp = T.n;
    const int Wa = cfg.acc_window, Wj = cfg.jerk_window;
    const double ehl = cfg.ego_length / 2, ehw = cfg.ego_width / 2;
    const double chl = cfg.car_length / 2, chw = cfg.car_width / 2;

    const int steps0 = st.steps[s];
    uint32_t flags;
    int cnt0, cnt1, cnt2, cnt3, cnt4, fs0, fs1, fs2, fs3, fs4;
    int first_car, hint, off_run;
    double hx, hy, dist, clean, min_sep, max_mph, max_acc, max_jerk;
    if (steps0 == 0) {                      // fresh episode
        flags = 0;
        cnt0 = cnt1 = cnt2 = cnt3 = cnt4 = 0;
        fs0 = fs1 = fs2 = fs3 = fs4 = 0;
        first_car = 0; hint = -1; off_run = 0;
        const double a = yaw_deg * 3.14159265358979323846 / 180;
        if (!ppg::cos(a, hx) || !ppg::sin(a, hy)) { hx = 1.0; hy = 0.0; }   // absurd yaw: along +x
        dist = 0; clean = 0; min_sep = INFINITY; max_mph = 0; max_acc = 0; max_jerk = 0;
        st.ring_vx[s] = 0.0; st.ring_vy[s] = 0.0;                          // v_0 = 0
    } else {
        flags = st.flags[s];
        cnt0 = st.count[0 * S + s]; cnt1 = st.count[1 * S + s]; cnt2 = st.count[2 * S + s];
        cnt3 = st.count[3 * S + s]; cnt4 = st.count[4 * S + s];
        fs0 = st.first_step[0 * S + s]; fs1 = st.first_step[1 * S + s]; fs2 = st.first_step[2 * S + s];
        fs3 = st.first_step[3 * S + s]; fs4 = st.first_step[4 * S + s];
        first_car = st.first_car[s]; hint = st.seg_hint[s]; off_run = st.off_run[s];
        hx = st.head_x[s]; hy = st.head_y[s];
        dist = st.dist[s]; clean = st.clean_dist[s]; min_sep = st.min_sep[s];
        max_mph = st.max_speed_mph[s]; max_acc = st.max_acc[s]; max_jerk = st.max_jerk[s];
    }

    const int kk = n_out < consume ? n_out : consume;
    double ppx = x0, ppy = y0;              // p_{i-1}
    for (int i = 1; i <= consume; i++) {
        const int n = steps0 + i;           // the episode's step number
        double px = ppx, py = ppy;          // the ego stands still once the plan runs out
        if (i <= kk) { px = next_x[(int64_t)(i - 1) * S + s]; py = next_y[(int64_t)(i - 1) * S + s]; }
        const double dx = px - ppx, dy = py - ppy;
        const double len = sqrt(dx * dx + dy * dy);
        const double vx = dx / kDt, vy = dy / kDt;
        const double mph = sqrt(vx * vx + vy * vy) * 2.237;
        dist += len;
        if (len > 0) { hx = dx / len; hy = dy / len; }
        st.ring_vx[(int64_t)(n & kRingMask) * S + s] = vx;
        st.ring_vy[(int64_t)(n & kRingMask) * S + s] = vy;
        const bool v_speed = mph > cfg.speed_limit_mph;
        if (mph > max_mph) max_mph = mph;

        // windowed acceleration and jerk from the ring
        bool v_acc = false, v_jerk = false;
        if (n >= Wa) {
            const int64_t ia = (int64_t)((n - Wa) & kRingMask) * S + s;
            const double ax = (vx - st.ring_vx[ia]) / (Wa * kDt), ay = (vy - st.ring_vy[ia]) / (Wa * kDt);
            const double acc = sqrt(ax * ax + ay * ay);
            v_acc = acc > cfg.max_acc;
            if (acc > max_acc) max_acc = acc;
            if (n >= Wa + Wj) {
                const int64_t ib = (int64_t)((n - Wj) & kRingMask) * S + s;
                const int64_t ic = (int64_t)((n - Wj - Wa) & kRingMask) * S + s;
                const double bx = (st.ring_vx[ib] - st.ring_vx[ic]) / (Wa * kDt);
                const double by = (st.ring_vy[ib] - st.ring_vy[ic]) / (Wa * kDt);
                const double jx = (ax - bx) / (Wj * kDt), jy = (ay - by) / (Wj * kDt);
                const double jerk = sqrt(jx * jx + jy * jy);
                v_jerk = jerk > cfg.max_jerk;
                if (jerk > max_jerk) max_jerk = jerk;
            }
        }

        // collision: every car, advanced from the frame's start by i steps
        bool v_col = false;
        for (int j = 0; j < tr.n; j++) {
            const int64_t tx = (int64_t)j * S + s;
            const int lane = tr.lane[tx];
            int seg = tr.seg[tx];
            double t = tr.t[tx];
            const double v = tr.v[tx];
            ppsynth::lane_advance(T, lane, &seg, &t, v * 0.02 * i);
            double cx, cy, cvx, cvy;
            ppsynth::traffic_car(T, lane, seg, t, tr.off[tx], v, &cx, &cy, &cvx, &cvy);
            const double ux = T.tan_x[lane * n_wp + seg], uy = T.tan_y[lane * n_wp + seg];
            const double sep = rect_sep(px, py, hx, hy, ehl, ehw, cx, cy, ux, uy, chl, chw);
            if (sep < min_sep) min_sep = sep;
            if (sep <= 0) {
                if (!v_col && !(flags & PP_INC_COLLISION)) first_car = j + 1;
                v_col = true;
            }
        }

        // off-lane: nearest lane-centre segment, searched around the carried hint
        const bool full = n == 1 || hint < 0 || hint >= n_wp;
        const int k0 = full ? 0 : -2, k1 = full ? n_wp - 1 : 2;
        double best = INFINITY;
        int best_seg = full ? 0 : hint;
        for (int lane = 0; lane < PP_NUM_LANES; lane++) {
            for (int k = k0; k <= k1; k++) {
                int seg = k;
                if (!full) {
                    seg = hint + k;
                    seg = seg < 0 ? seg + n_wp : (seg >= n_wp ? seg - n_wp : seg);   // n_wp >= 3
                }
                const double d2 = seg_dist2(T, lane, seg, px, py);
                if (d2 < best) { best = d2; best_seg = seg; }
            }
        }
        hint = best_seg;
        off_run = sqrt(best) > cfg.lane_tol ? off_run + 1 : 0;
        const bool v_off = off_run > cfg.off_lane_steps;

        // records
        if (v_col) { cnt0++; if (!fs0) fs0 = n; flags |= PP_INC_COLLISION; }
        if (v_speed) { cnt1++; if (!fs1) fs1 = n; flags |= PP_INC_SPEED; }
        if (v_acc) { cnt2++; if (!fs2) fs2 = n; flags |= PP_INC_ACC; }
        if (v_jerk) { cnt3++; if (!fs3) fs3 = n; flags |= PP_INC_JERK; }
        if (v_off) { cnt4++; if (!fs4) fs4 = n; flags |= PP_INC_OFF_LANE; }
        if (!flags) clean = dist;
        ppx = px; ppy = py;
    }

    st.steps[s] = steps0 + consume;
    st.flags[s] = flags;
    st.count[0 * S + s] = cnt0; st.count[1 * S + s] = cnt1; st.count[2 * S + s] = cnt2;
    st.count[3 * S + s] = cnt3; st.count[4 * S + s] = cnt4;
    st.first_step[0 * S + s] = fs0; st.first_step[1 * S + s] = fs1; st.first_step[2 * S + s] = fs2;
    st.first_step[3 * S + s] = fs3; st.first_step[4 * S + s] = fs4;
    st.first_car[s] = first_car; st.seg_hint[s] = hint; st.off_run[s] = off_run;
    st.head_x[s] = hx; st.head_y[s] = hy;
    st.dist[s] = dist; st.clean_dist[s] = clean; st.min_sep[s] = min_sep;
    st.max_speed_mph[s] = max_mph; st.max_acc[s] = max_acc; st.max_jerk[s] = max_jerk;
}

}  // namespace ppjudge
