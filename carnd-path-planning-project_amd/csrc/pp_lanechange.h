// pp_lanechange.h — lane-changing traffic (include/pp.h pp_traffic_lane_change; DESIGN.md "Lane-changing
// traffic").
//
// One function lets the traffic of one scene change lanes for one frame, by MOBIL ("minimising overall
// braking induced by lane changes") on the IDM accelerations of pp_follow.h: a car moves to a
// neighbour lane when that is safe for it and for its new follower and when what it gains, plus
// `politeness` times what its new and its old follower gain, exceeds a threshold. It runs after the
// follow update of the same frame and reads that update's records (desired speeds, leaders, net gaps,
// the ego's segment) and speeds; it writes the cars' lane, seg, t and offset and its own state, never
// a speed. At most one car per scene begins a change per call. The definitions are this project's own
// (the reference has no simulator: nothing here is compared with it). Compiled for the device
// (k_lane_change) and the host (pp_traffic_lane_change_host): only + - * / sqrt on the same inputs in
// the same order, under -ffp-contract=off on both sides, so the two agree bit for bit.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "../../include/pp.h"
#include "pp_synth.h"
#include "pp_follow.h"

namespace pplanechange {

// pp_lane_change_cfg_default's values (host only)
inline void cfg_default(pp_lane_change_cfg* c) {
    memset(c, 0, sizeof(*c));
    c->politeness = 0.3;
    c->threshold = 0.2;
    c->right_bias = 0.0;
    c->safe_brake = 3.0;
    c->lateral_speed = 1.5;
    c->ego_desired_speed = 22.2;
    c->min_interval_steps = 250;
}

PP_HD inline bool cfg_ok(const pp_lane_change_cfg& c) {
    return c.politeness >= 0 && c.threshold == c.threshold && c.right_bias == c.right_bias && c.safe_brake > 0 &&
           c.lateral_speed > 0 && c.ego_desired_speed > 0 && c.min_interval_steps >= 0;
}

// pp_follow.h's acceleration (follow_scene pass 3, restated): v0 > 0; two_sab = 2 sqrt(max_acc comfort_brake)
PP_HD inline double idm(const pp_follow_cfg& F, double two_sab, double v, double v0, bool lead, double vl, double g) {
    const double r = v / v0;
    const double free = 1 - (r * r) * (r * r);
    double a = F.max_acc * free;
    if (lead) {
        const double dyn = v * F.time_headway + v * (v - vl) / two_sab;
        const double sstar = F.min_gap + (dyn > 0 ? dyn : 0.0);
        const double q = sstar / (g > F.gap_floor ? g : F.gap_floor);
        a = F.max_acc * (free - q * q);
    }
    return a < -F.max_brake ? -F.max_brake : a;
}

// Car m's acceleration behind the leader the follow update recorded for it (v0 = its desired speed > 0).
PP_HD inline double idm_recorded(const pp_follow_cfg& F, double two_sab, int64_t S, int64_t s, int J, double ve,
                                 const ppsynth::TrafficV& tr, const pp_follow& fs, int m, double v0) {
    const int64_t mx = (int64_t)m * S + s;
    const int lead = fs.leader[mx];
    const double vl = lead < 0 ? 0.0 : (lead == J ? ve : tr.v[(int64_t)lead * S + s]);
    return idm(F, two_sab, tr.v[mx], v0, lead >= 0, vl, fs.gap[mx]);
}

// Where a car standing at (lane, seg, t, off) comes to lie on lane `to`: the nearest of the segments
// seg - 1, seg, seg + 1 of that lane (the first strictly smaller squared distance wins), the clamped
// fraction on it and the offset along its right-hand normal (ppfollow::seg_project's projection,
// keeping the foot).
PP_HD inline void place_on(const ppsynth::LaneTables& T, int lane, int seg, double t, double off, int to,
                           int* oseg, double* ot, double* ooff) {
    const int n = T.n;
    double px, py, vx, vy;
    ppsynth::traffic_car(T, lane, seg, t, off, 0.0, &px, &py, &vx, &vy);
    double best = INFINITY, bt = 0, bdx = 0, bdy = 0;
    int bs = seg;
    for (int k = -1; k <= 1; k++) {
        int sg = seg + k;
        sg = sg < 0 ? sg + n : (sg >= n ? sg - n : sg);                        // n >= 3
        const int ip = (sg == 0) ? n - 1 : sg - 1;
        const double ax = T.lc_x[to * n + ip], ay = T.lc_y[to * n + ip];
        const double bx = T.lc_x[to * n + sg], by = T.lc_y[to * n + sg];
        const double ex = bx - ax, ey = by - ay;
        const double ee = ex * ex + ey * ey;
        double u = ee > 0 ? ((px - ax) * ex + (py - ay) * ey) / ee : 0.0;
        u = u < 0 ? 0.0 : (u > 1 ? 1.0 : u);
        const double dx = px - (ax + ex * u), dy = py - (ay + ey * u);
        const double d2 = dx * dx + dy * dy;
        if (d2 < best) { best = d2; bs = sg; bt = u; bdx = dx; bdy = dy; }
    }
    *oseg = bs;
    *ot = bt;
    *ooff = bdx * T.tan_y[to * n + bs] - bdy * T.tan_x[to * n + bs];
}

// One frame of scene s (all arrays [k * S + s]). (ex, ey), ego_mph: the ego before the frame; tr: the
// traffic before the frame with the speeds the follow update has just written; fs: that update's
// state (read only); st: the scene's carried lane-change state and records. Per-car values with a
// runtime index are staged in global memory (st.arc); the candidates are worked on kBlock cars at a
// time, two directions each, in arrays that only fully unrolled loops index (registers), so every
// other car is read once per block, not once per pair. A short last block repeats the last car and
// discards the repeats.
constexpr int kBlock = 2;
PP_HD inline void lane_change_scene(const ppsynth::LaneTables& T, const ppfollow::ArcTables& A, int64_t S, int64_t s,
                                    double ex, double ey, double ego_mph, const ppsynth::TrafficV& tr, int consume,
                                    const pp_follow_cfg& F, const pp_follow& fs, const pp_lane_change_cfg& cfg,
                                    const pp_lane_change& st) {
    if (fs.started[s] == 0) return;               // the follow update has not seen this scene: not ours
    const int n_wp = T.n;
    const int J = tr.n;

    if (st.started[s] == 0) {                     // fresh episode
        for (int j = 0; j < J; j++) {
            const int64_t tx = (int64_t)j * S + s;
            st.home[tx] = tr.off[tx];
            st.wait[tx] = 0;
            st.changes[tx] = 0;
        }
        st.n_changes[s] = 0;
        st.started[s] = 1;
    }

    // every car: the offset returns to its home value, the wait runs down; the arcs
    const double dt = consume * 0.02;
    const double step = cfg.lateral_speed * dt;
    for (int j = 0; j < J; j++) {
        const int64_t tx = (int64_t)j * S + s;
        const double home = st.home[tx], off = tr.off[tx];
        const double d = home - off;
        tr.off[tx] = (d < 0 ? -d : d) <= step ? home : off + (d > 0 ? step : -step);
        const int w = st.wait[tx] - consume;
        st.wait[tx] = w > 0 ? w : 0;
        st.arc[tx] = ppfollow::arc_of(T, A, tr.lane[tx], tr.seg[tx], tr.t[tx]);
    }

    // the ego on every lane, as follow_scene finds it, around the segment that call has just written
    const int hint = fs.ego_seg[s] - 1;
    const bool full = hint < 0 || hint >= n_wp;
    const int k0 = full ? 0 : -2, k1 = full ? n_wp - 1 : 2;
    double arc_e[PP_NUM_LANES];
    bool occ[PP_NUM_LANES];
#pragma unroll
    for (int lane = 0; lane < PP_NUM_LANES; lane++) {
        double bl = INFINITY, bt = 0;
        int bs = full ? 0 : hint;
        for (int k = k0; k <= k1; k++) {
            int seg = k;
            if (!full) {
                seg = hint + k;
                seg = seg < 0 ? seg + n_wp : (seg >= n_wp ? seg - n_wp : seg);   // n_wp >= 3
            }
            double t;
            const double d2 = ppfollow::seg_project(T, lane, seg, ex, ey, &t);
            if (d2 < bl) { bl = d2; bs = seg; bt = t; }
        }
        arc_e[lane] = ppfollow::arc_of(T, A, lane, bs, bt);
        occ[lane] = F.react_to_ego && sqrt(bl) <= F.lateral_reach;
    }
    const double ve = ego_mph / 2.237;
    const double two_sab = 2 * sqrt(F.max_acc * F.comfort_brake);

    // candidates: slot q = 2 k + d of a block is car j0 + k moving to lane - 1 (d = 0) or lane + 1 (d = 1)
    constexpr int kSlots = 2 * kBlock;
    double win = 0;
    int win_j = -1, win_dir = 0;
    for (int j0 = 0; j0 < J; j0 += kBlock) {
        bool elig[kBlock];
        int old[kBlock];
        double vj[kBlock], v0j[kBlock], acc[kBlock], gapj[kBlock], vlead[kBlock];
        int to[kSlots], lead[kSlots], foll[kSlots];
        double ap[kSlots], loop[kSlots], gn[kSlots], gf[kSlots];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const bool real = j0 + k < J;
            const int64_t tx = (int64_t)(real ? j0 + k : J - 1) * S + s;
            const int lane = tr.lane[tx], seg = tr.seg[tx];
            const double t = tr.t[tx], off = tr.off[tx];
            v0j[k] = fs.desired[tx];
            vj[k] = tr.v[tx];
            gapj[k] = fs.gap[tx];
            const int ld = fs.leader[tx];
            vlead[k] = ld < 0 ? 0.0 : (ld == J ? ve : tr.v[(int64_t)ld * S + s]);
            elig[k] = real && v0j[k] > 0 && st.wait[tx] == 0 && off == st.home[tx];
            acc[k] = elig[k] ? idm(F, two_sab, vj[k], v0j[k], ld >= 0, vlead[k], gapj[k]) : 0.0;
            if (ld < 0) gapj[k] = INFINITY;
            old[k] = -1;
#pragma unroll
            for (int d = 0; d < 2; d++) {
                const int q = 2 * k + d;
                const int l2 = lane + (d ? 1 : -1);
                const bool ok = elig[k] && l2 >= 0 && l2 < PP_NUM_LANES;
                to[q] = ok ? l2 : -1;
                ap[q] = 0;
                loop[q] = 0;
                gn[q] = gf[q] = INFINITY;
                lead[q] = foll[q] = -1;
                if (ok) {
                    int sg;
                    double t2, off2;
                    place_on(T, lane, seg, t, off, l2, &sg, &t2, &off2);
                    ap[q] = ppfollow::arc_of(T, A, l2, sg, t2);
                    double ae = 0;
                    bool oe = false;
#pragma unroll
                    for (int l = 0; l < PP_NUM_LANES; l++)
                        if (l2 == l) { ae = arc_e[l]; oe = occ[l]; loop[q] = A.loop[l]; }
                    if (oe) {
                        double c = ae - ap[q];
                        if (c < 0) c += loop[q];
                        gn[q] = c;
                        c = ap[q] - ae;
                        if (c <= 0) c += loop[q];
                        gf[q] = c;
                        lead[q] = foll[q] = J;
                    }
                }
            }
        }
        // every other car once per block: new leaders and followers (the ego first, then ascending
        // index), and each car's old follower (the lowest car whose recorded leader it is)
        for (int m = 0; m < J; m++) {
            const int64_t mx = (int64_t)m * S + s;
            const int lm = tr.lane[mx];
            const int ldm = fs.leader[mx];
            const double am = st.arc[mx];
#pragma unroll
            for (int k = 0; k < kBlock; k++)
                if (ldm == j0 + k && old[k] < 0) old[k] = m;
#pragma unroll
            for (int q = 0; q < kSlots; q++) {
                const bool hit = m != j0 + (q >> 1) && lm == to[q];
                double cn = am - ap[q];
                if (cn < 0) cn += loop[q];
                double cf = ap[q] - am;
                if (cf <= 0) cf += loop[q];
                if (hit && cn < gn[q]) { gn[q] = cn; lead[q] = m; }
                if (hit && cf < gf[q]) { gf[q] = cf; foll[q] = m; }
            }
        }
        // the surplus of every slot, the block's records, the scene's best so far
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            double sur[2] = {-INFINITY, -INFINITY};
            // the old follower's gain does not depend on the direction
            double d_old = 0;
            if (elig[k] && old[k] >= 0) {
                const int64_t ox = (int64_t)old[k] * S + s;
                const double v0o = fs.desired[ox];
                if (v0o > 0) {
                    const double vo = tr.v[ox], go = fs.gap[ox];
                    const double a_o = idm(F, two_sab, vo, v0o, true, vj[k], go);
                    const double g2 = go + gapj[k] + F.car_length;
                    const double a_o2 = idm(F, two_sab, vo, v0o, !(g2 > F.horizon), vlead[k], g2);
                    d_old = a_o2 - a_o;
                }
            }
#pragma unroll
            for (int d = 0; d < 2; d++) {
                const int q = 2 * k + d;
                if (to[q] < 0) continue;
                bool safe = true;
                // the new leader
                bool has_n = lead[q] >= 0;
                double g_n = INFINITY, v_n = 0;
                if (has_n) {
                    g_n = gn[q] - (F.car_length + (lead[q] == J ? F.ego_length : F.car_length)) / 2;
                    if (g_n > F.horizon) has_n = false;
                    else {
                        v_n = lead[q] == J ? ve : tr.v[(int64_t)lead[q] * S + s];
                        safe = safe && g_n >= F.min_gap;
                    }
                }
                const double a_j2 = idm(F, two_sab, vj[k], v0j[k], has_n, v_n, g_n);
                safe = safe && a_j2 >= -cfg.safe_brake;
                // the new follower
                double d_foll = 0;
                if (foll[q] >= 0) {
                    const double g_f = gf[q] - ((foll[q] == J ? F.ego_length : F.car_length) + F.car_length) / 2;
                    if (!(g_f > F.horizon)) {
                        safe = safe && g_f >= F.min_gap;
                        double a_f2 = 0;                                       // (a parked follower)
                        if (foll[q] == J) {
                            a_f2 = idm(F, two_sab, ve, cfg.ego_desired_speed, true, vj[k], g_f);
                        } else {
                            const int64_t fx = (int64_t)foll[q] * S + s;
                            const double v0f = fs.desired[fx];
                            if (v0f > 0) {
                                a_f2 = idm(F, two_sab, tr.v[fx], v0f, true, vj[k], g_f);
                                d_foll = a_f2 - idm_recorded(F, two_sab, S, s, J, ve, tr, fs, foll[q], v0f);
                            }
                        }
                        safe = safe && a_f2 >= -cfg.safe_brake;
                    }
                }
                if (safe) {
                    const double gain = (a_j2 - acc[k]) + cfg.politeness * (d_foll + d_old);
                    sur[d] = gain - cfg.threshold - (d ? -cfg.right_bias : cfg.right_bias);
                }
            }
            if (j0 + k >= J) continue;
            const int dir = sur[1] > sur[0] ? 1 : -1;
            const double best = sur[1] > sur[0] ? sur[1] : sur[0];
            const int64_t tx = (int64_t)(j0 + k) * S + s;
            st.gain[tx] = elig[k] ? best : -INFINITY;
            st.dir[tx] = elig[k] && best > -INFINITY ? dir : 0;
            if (elig[k] && best > win) { win = best; win_j = j0 + k; win_dir = dir; }
        }
    }

    // at most one change per scene and call, written last
    st.last_car[s] = win_j + 1;
    st.last_dir[s] = win_dir;
    if (win_j >= 0) {
        const int64_t tx = (int64_t)win_j * S + s;
        const int lane = tr.lane[tx];
        int sg;
        double t2, off2;
        place_on(T, lane, tr.seg[tx], tr.t[tx], tr.off[tx], lane + win_dir, &sg, &t2, &off2);
        tr.lane[tx] = lane + win_dir;
        tr.seg[tx] = sg;
        tr.t[tx] = t2;
        tr.off[tx] = off2;
        st.wait[tx] = cfg.min_interval_steps;
        st.changes[tx] = st.changes[tx] + 1;
        st.n_changes[s] = st.n_changes[s] + 1;
    }
}

}  // namespace pplanechange
