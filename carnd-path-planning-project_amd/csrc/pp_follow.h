// pp_follow.h — car-following traffic (include/pp.h pp_traffic_follow; DESIGN.md "Reactive traffic").
//
// One function updates the speeds of one scene's traffic for one frame: every car follows the
// vehicle ahead of it in its lane (another car, or the ego where it occupies the lane) by the
// Intelligent Driver Model. It reads the pre-frame ego pose and speed and the pre-frame traffic and
// nothing of the plan. The definitions are this project's own (the reference has no simulator:
// nothing here is compared with it). Compiled for the device (k_follow) and the host
// (pp_traffic_follow_host): only + - * / sqrt on the same inputs in the same order, under
// -ffp-contract=off on both sides, so the two agree bit for bit.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "../../include/pp.h"
#include "pp_synth.h"

namespace ppfollow {

// Arc-length prefix of the lane polylines (built once per map on the host from LaneTables::seg_len
// by one left-to-right sum; the device reads an uploaded copy of the same bits).
struct ArcTables {
    const double* cum;    // [lane * n + i] sum of seg_len[lane][0..i): the arc at the start of segment i
    const double* loop;   // [lane] the whole ring
};
inline size_t arc_doubles(int n) { return (size_t)PP_NUM_LANES * n + PP_NUM_LANES; }
inline void build_arc(const double* seg_len, int n, double* out) {
    for (int l = 0; l < PP_NUM_LANES; l++) {
        double a = 0;
        for (int i = 0; i < n; i++) { out[l * n + i] = a; a += seg_len[l * n + i]; }
        out[PP_NUM_LANES * n + l] = a;
    }
}
inline ArcTables arc_tables(const double* t, int n) {
    ArcTables A;
    A.cum = t; A.loop = t + PP_NUM_LANES * n;
    return A;
}

// pp_follow_cfg_default's values (host only)
inline void cfg_default(pp_follow_cfg* c) {
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

PP_HD inline bool cfg_ok(const pp_follow_cfg& c) {
    return c.max_acc > 0 && c.comfort_brake > 0 && c.max_brake > 0 && c.gap_floor > 0 && c.horizon >= 0 &&
           c.car_length >= 0 && c.ego_length >= 0 && c.lateral_reach >= 0;
}

PP_HD inline double arc_of(const ppsynth::LaneTables& T, const ArcTables& A, int lane, int seg, double t) {
    return A.cum[lane * T.n + seg] + t * T.seg_len[lane * T.n + seg];
}

// Squared distance from p to segment `seg` of lane `lane` and the clamped fraction *t of its
// nearest point (ppjudge::seg_dist2's projection, keeping t).
PP_HD inline double seg_project(const ppsynth::LaneTables& T, int lane, int seg, double px, double py, double* t) {
    const int n = T.n;
    const int ip = (seg == 0) ? n - 1 : seg - 1;
    const double ax = T.lc_x[lane * n + ip], ay = T.lc_y[lane * n + ip];
    const double bx = T.lc_x[lane * n + seg], by = T.lc_y[lane * n + seg];
    const double ex = bx - ax, ey = by - ay;
    const double ee = ex * ex + ey * ey;
    double u = ee > 0 ? ((px - ax) * ex + (py - ay) * ey) / ee : 0.0;
    u = u < 0 ? 0.0 : (u > 1 ? 1.0 : u);
    const double qx = px - (ax + ex * u), qy = py - (ay + ey * u);
    *t = u;
    return qx * qx + qy * qy;
}

// Updates tr.v of scene s for one frame of `consume` steps (all arrays [k * S + s]). (ex, ey),
// ego_mph: the ego before the frame; tr: the traffic before the frame (only v is written); st: the
// scene's carried state and records. Four passes over the cars, staged in global memory (a per-car
// array with a runtime index would live in scratch): the arcs (into next_speed), the leaders and
// net gaps from the arcs, the new speeds from the pre-frame speeds (into next_speed: the Jacobi
// update), the write-back. The kernel is bound by the latency of its dependent global reads, so
// passes 1 and 2 work on kBlock cars at a time, held in arrays that only fully unrolled loops index
// (registers): a block's reads go out together, and pass 2 reads every other car once per block, not
// once per pair. A short last block repeats the last car and discards the repeats.
constexpr int kBlock = 4;
PP_HD inline void follow_scene(const ppsynth::LaneTables& T, const ArcTables& A, int64_t S, int64_t s, double ex,
                               double ey, double ego_mph, const ppsynth::TrafficV& tr, int consume,
                               const pp_follow_cfg& cfg, const pp_follow& st) {
    const int n_wp = T.n;
    const int J = tr.n;
    const bool fresh = st.started[s] == 0;

    // the ego on every lane: nearest point of the lane's centre polyline, around the carried hint
    const int hint = fresh ? -1 : st.ego_seg[s] - 1;
    const bool full = hint < 0 || hint >= n_wp;
    const int k0 = full ? 0 : -2, k1 = full ? n_wp - 1 : 2;
    double arc_e[PP_NUM_LANES];
    bool occ[PP_NUM_LANES];
    double best = INFINITY;
    int best_seg = full ? 0 : hint;
#pragma unroll
    for (int lane = 0; lane < PP_NUM_LANES; lane++) {
        double bl = INFINITY, bt = 0;
        int bs = best_seg;
        for (int k = k0; k <= k1; k++) {
            int seg = k;
            if (!full) {
                seg = hint + k;
                seg = seg < 0 ? seg + n_wp : (seg >= n_wp ? seg - n_wp : seg);   // n_wp >= 3
            }
            double t;
            const double d2 = seg_project(T, lane, seg, ex, ey, &t);
            if (d2 < bl) { bl = d2; bs = seg; bt = t; }
        }
        arc_e[lane] = arc_of(T, A, lane, bs, bt);
        occ[lane] = cfg.react_to_ego && sqrt(bl) <= cfg.lateral_reach;
        if (bl < best) { best = bl; best_seg = bs; }
    }
    const double ve = ego_mph / 2.237;

    // pass 1: arcs (and, on a fresh episode, the desired speeds)
    for (int j0 = 0; j0 < J; j0 += kBlock) {
        int ln[kBlock], sg[kBlock];
        double tt[kBlock], arc[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int64_t tx = (int64_t)(j0 + k < J ? j0 + k : J - 1) * S + s;
            ln[k] = tr.lane[tx]; sg[k] = tr.seg[tx]; tt[k] = tr.t[tx];
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) arc[k] = arc_of(T, A, ln[k], sg[k], tt[k]);
#pragma unroll
        for (int k = 0; k < kBlock; k++)
            if (j0 + k < J) st.next_speed[(int64_t)(j0 + k) * S + s] = arc[k];
    }
    if (fresh)
        for (int j = 0; j < J; j++) st.desired[(int64_t)j * S + s] = tr.v[(int64_t)j * S + s];

    // pass 2: leaders and net gaps, kBlock cars at a time against every other car (whose lane and arc
    // are then read once per block). Rank: the ego first, then ascending car index.
    for (int j0 = 0; j0 < J; j0 += kBlock) {
        int lane[kBlock], lead[kBlock];
        double aj[kBlock], loop[kBlock], gc[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const int64_t tx = (int64_t)(j0 + k < J ? j0 + k : J - 1) * S + s;
            lane[k] = tr.lane[tx];
            aj[k] = st.next_speed[tx];
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            loop[k] = A.loop[lane[k]];
            double ae = 0;
            bool oe = false;
#pragma unroll
            for (int l = 0; l < PP_NUM_LANES; l++)
                if (lane[k] == l) { ae = arc_e[l]; oe = occ[l]; }
            gc[k] = INFINITY;
            lead[k] = -1;
            if (oe) {
                gc[k] = ae - aj[k];
                if (gc[k] < 0) gc[k] += loop[k];
                lead[k] = J;
            }
        }
        for (int m = 0; m < J; m++) {
            const int64_t mx = (int64_t)m * S + s;
            const int lm = tr.lane[mx];
            const double am = st.next_speed[mx];
#pragma unroll
            for (int k = 0; k < kBlock; k++) {
                double c = am - aj[k];
                if (c < 0 || (c == 0 && m > j0 + k)) c += loop[k];
                if (m != j0 + k && lm == lane[k] && c < gc[k]) { gc[k] = c; lead[k] = m; }
            }
        }
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            if (j0 + k >= J) continue;
            double g = INFINITY;
            if (lead[k] >= 0) {
                g = gc[k] - (cfg.car_length + (lead[k] == J ? cfg.ego_length : cfg.car_length)) / 2;
                if (g > cfg.horizon) { g = INFINITY; lead[k] = -1; }
            }
            st.leader[(int64_t)(j0 + k) * S + s] = lead[k];
            st.gap[(int64_t)(j0 + k) * S + s] = g;
        }
    }

    // pass 3: IDM from the pre-frame speeds, staged (the arcs are no longer needed)
    const double dt = consume * 0.02;
    const double two_sab = 2 * sqrt(cfg.max_acc * cfg.comfort_brake);
    for (int j = 0; j < J; j++) {
        const int64_t tx = (int64_t)j * S + s;
        const double v = tr.v[tx], v0 = st.desired[tx];
        double vn = v;
        if (v0 > 0) {                               // (a parked car is left unchanged)
            const double r = v / v0;
            const double free = 1 - (r * r) * (r * r);
            const int lead = st.leader[tx];
            double a = cfg.max_acc * free;
            if (lead >= 0) {
                const double vl = lead == J ? ve : tr.v[(int64_t)lead * S + s];
                const double dyn = v * cfg.time_headway + v * (v - vl) / two_sab;
                const double sstar = cfg.min_gap + (dyn > 0 ? dyn : 0.0);
                const double g = st.gap[tx];
                const double q = sstar / (g > cfg.gap_floor ? g : cfg.gap_floor);
                a = cfg.max_acc * (free - q * q);
            }
            if (a < -cfg.max_brake) a = -cfg.max_brake;
            vn = v + a * dt;
            vn = vn > 0 ? vn : 0.0;
            vn = vn < v0 ? vn : v0;
        }
        st.next_speed[tx] = vn;
    }

    // pass 4: write back
    for (int j = 0; j < J; j++) {
        const int64_t tx = (int64_t)j * S + s;
        tr.v[tx] = st.next_speed[tx];
    }
    st.started[s] = 1;
    st.ego_seg[s] = best_seg + 1;
}

}  // namespace ppfollow
