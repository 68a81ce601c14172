// pp_tracker.h — the tracker between the sensor and the planner (include/pp.h pp_track_frame;
// DESIGN.md §20 "Tracker"). THIS LIBRARY'S OWN definitions; the reference has no tracker.
//
// One PP_HD function, track_scene, behind the kernel (k_track) and the host twin. It uses only
// + - * /, IEEE sqrt and integer arithmetic, and both sides are compiled with -ffp-contract=off, so
// device and host agree bit for bit. The rows (the sensor state's, or the telemetry's truth) are only
// read; tracks and tracked rows go to the tracker state's own arrays.
//
// Sensor fusion gives stable ids, so a scene is one merge in id order of its old tracks (bank f & 1
// of the state, f = frame[s]; empty when f == 0) with its accepted rows (row r < n = clamp(n_cars, 0,
// K) whose id is greater than the last accepted row's), written to the other bank. Per axis the state
// is (position, velocity) under a constant-velocity model; both axes share one covariance
// (ppp, ppv, pvv). Every formula is evaluated in exactly the order written, left to right:
//   constants  d2 = dt dt, q = acc_sigma acc_sigma, q4 = (q (d2 d2)) / 4, q3 = (q (d2 dt)) / 2, q2 = q d2,
//              rvv = meas_vel_sigma meas_vel_sigma
//   predict    (every old track, from its stored values) x = x + dt vx, y = y + dt vy,
//              ppp' = (ppp + dt ((2 ppv) + (dt pvv))) + q4, ppv' = (ppv + dt pvv) + q3, pvv' = pvv + q2
//   R of a row a = (zx - ex, zy - ey), sp = meas_pos_sigma + meas_pos_sigma_per_m sqrt(ax ax + ay ay)
//              (exactly 0 where both coefficients are 0, whatever a), rpp = sp sp
//   id in both (UPDATED, misses = 0) spp = ppp + rpp, spv = ppv, svv = pvv + rvv, det = spp svv - spv spv;
//              innovations ix = zx - x, ivx = zvx - vx, iy = zy - y, ivy = zvy - vy.
//              The row is taken outright (state = z, covariance (rpp, 0, rvv)) when rpp == 0 && rvv == 0,
//              or !(det > 0), or det or an innovation is not finite (an innovation is finite only where
//              the row's field is). Otherwise
//                k11 = (ppp svv - ppv spv) / det   k12 = (ppv spp - ppp spv) / det
//                k21 = (ppv svv - pvv spv) / det   k22 = (pvv spp - ppv spv) / det
//                x = x + (k11 ix + k12 ivx), vx = vx + (k21 ix + k22 ivx), the same for y with iy, ivy
//                ppp'' = ppp - (k11 ppp + k12 ppv), ppv'' = ppv - (k11 ppv + k12 pvv),
//                pvv'' = pvv - (k21 ppv + k22 pvv)          (right-hand sides: the predicted values)
//   row only   (NEW) state = z, covariance (rpp, 0, rvv), misses = 0
//   track only deleted when misses >= max_coast (misses + 1 > max_coast) or when it does not leave room
//              for the rows still to come: kept only while out + (n - r) < K, out tracks written and r
//              rows consumed so far (skipped rows count as consumed once passed). A kept track is
//              COASTED, misses + 1, its row the predicted state: a straight line, not a lane.
// Reported rows always fit: out + (n - r) <= K holds throughout.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "pp_sensor.h"

namespace pptracker {

// pp_tracker_cfg_default's values (host only): the identity tracker
inline void cfg_default(pp_tracker_cfg* c) { memset(c, 0, sizeof(*c)); }

PP_HD inline bool cfg_ok(const pp_tracker_cfg& c) {
    return ppsensor::amount_ok(c.meas_pos_sigma) && ppsensor::amount_ok(c.meas_pos_sigma_per_m) &&
           ppsensor::amount_ok(c.meas_vel_sigma) && ppsensor::amount_ok(c.acc_sigma) && c.max_coast >= 0;
}

PP_HD inline bool finite(double x) { return x - x == 0; }

// Scene s of the batch `Z` (the rows as the sensor or the simulator left them): merges the state's
// old bank with the rows into the other bank, writes the tracked rows and advances the frame.
PP_HD inline void track_scene(const ppsensor::Truth& Z, int64_t s, const pp_tracker_cfg& cfg, double dt,
                              const pp_tracker& st) {
    const int64_t S = Z.S;
    const int K = Z.stride;
    int n = Z.n_cars[s];
    n = n < 0 ? 0 : (n > K ? K : n);
    const uint32_t f = (uint32_t)st.frame[s];
    const int64_t rb = (int64_t)(f & 1u) * K, wb = (int64_t)((f & 1u) ^ 1u) * K;   // first slots of the banks
    int nold = f == 0 ? 0 : st.n_tracks[(int64_t)(f & 1u) * S + s];
    nold = nold < 0 ? 0 : (nold > K ? K : nold);
    const double ex = Z.ego_x[s], ey = Z.ego_y[s];
    const double d2 = dt * dt, q = cfg.acc_sigma * cfg.acc_sigma;
    const double q4 = (q * (d2 * d2)) / 4.0, q3 = (q * (d2 * dt)) / 2.0, q2 = q * d2;
    const double rvv = cfg.meas_vel_sigma * cfg.meas_vel_sigma;
    const bool noisy_p = cfg.meas_pos_sigma != 0 || cfg.meas_pos_sigma_per_m != 0;
    int out = 0, r = 0, t = 0;
    int64_t last = INT64_MIN;                          // id of the last accepted row
    for (;;) {
        int32_t rid = 0;
        for (; r < n; r++) {                           // rows not in ascending id are passed over
            rid = Z.car_id[(int64_t)r * S + s];
            if ((int64_t)rid > last) break;
        }
        if (r >= n && t >= nold) break;
        const int64_t ti = (rb + t) * S + s, ri = (int64_t)r * S + s;
        const int32_t tid = t < nold ? st.id[ti] : 0;
        const bool has_row = r < n && (t >= nold || rid <= tid);
        const bool has_trk = t < nold && (r >= n || tid <= rid);
        double x = 0, y = 0, vx = 0, vy = 0, ppp = 0, ppv = 0, pvv = 0;
        int32_t misses = 0, src = PP_TRACK_NEW;
        if (has_trk) {
            const double ovx = st.vx[ti], ovy = st.vy[ti], oppp = st.ppp[ti], oppv = st.ppv[ti], opvv = st.pvv[ti];
            x = st.x[ti] + dt * ovx; y = st.y[ti] + dt * ovy;
            vx = ovx; vy = ovy;
            ppp = (oppp + dt * ((2.0 * oppv) + (dt * opvv))) + q4;
            ppv = (oppv + dt * opvv) + q3;
            pvv = opvv + q2;
            misses = st.misses[ti];
            t++;
        }
        if (has_row) {
            const double zx = Z.car_x[ri], zy = Z.car_y[ri], zvx = Z.car_vx[ri], zvy = Z.car_vy[ri];
            const double ax = zx - ex, ay = zy - ey;
            const double sp = noisy_p ? cfg.meas_pos_sigma + cfg.meas_pos_sigma_per_m * sqrt(ax * ax + ay * ay) : 0.0;
            const double rpp = sp * sp;
            bool outright = true;
            if (has_trk) {
                src = PP_TRACK_UPDATED;
                const double spp = ppp + rpp, spv = ppv, svv = pvv + rvv;
                const double det = spp * svv - spv * spv;
                const double ix = zx - x, ivx = zvx - vx, iy = zy - y, ivy = zvy - vy;
                if (!(rpp == 0 && rvv == 0) && det > 0 && finite(det) && finite(ix) && finite(ivx) && finite(iy) &&
                    finite(ivy)) {
                    outright = false;
                    const double k11 = (ppp * svv - ppv * spv) / det, k12 = (ppv * spp - ppp * spv) / det;
                    const double k21 = (ppv * svv - pvv * spv) / det, k22 = (pvv * spp - ppv * spv) / det;
                    x = x + (k11 * ix + k12 * ivx); vx = vx + (k21 * ix + k22 * ivx);
                    y = y + (k11 * iy + k12 * ivy); vy = vy + (k21 * iy + k22 * ivy);
                    const double nppp = ppp - (k11 * ppp + k12 * ppv), nppv = ppv - (k11 * ppv + k12 * pvv);
                    pvv = pvv - (k21 * ppv + k22 * pvv);
                    ppp = nppp; ppv = nppv;
                }
            }
            if (outright) { x = zx; y = zy; vx = zvx; vy = zvy; ppp = rpp; ppv = 0.0; pvv = rvv; }
            misses = 0;
            last = rid;
            r++;
        } else {
            // (r is at the next accepted row or at n: every row before it is consumed)
            if (misses >= cfg.max_coast || out + (n - r) >= K) continue;
            misses = misses + 1;
            src = PP_TRACK_COASTED;
        }
        const int32_t id = has_row ? rid : tid;
        const int64_t wi = (wb + out) * S + s, oi = (int64_t)out * S + s;
        st.id[wi] = id; st.misses[wi] = misses;
        st.x[wi] = x; st.y[wi] = y; st.vx[wi] = vx; st.vy[wi] = vy;
        st.ppp[wi] = ppp; st.ppv[wi] = ppv; st.pvv[wi] = pvv;
        st.car_id[oi] = id;
        st.car_x[oi] = x; st.car_y[oi] = y; st.car_vx[oi] = vx; st.car_vy[oi] = vy;
        st.src[oi] = src;
        out++;
    }
    for (int k = out; k < K; k++) st.src[(int64_t)k * S + s] = PP_TRACK_NONE;
    st.n_tracks[(int64_t)((f & 1u) ^ 1u) * S + s] = out;
    st.n_cars[s] = out;
    st.frame[s] = (int32_t)(f + 1u);
}

}  // namespace pptracker
