// pp_sensor.h — the sensor model between the world and the planner (include/pp.h pp_sense_frame;
// DESIGN.md §19 "Sensor model"). THIS LIBRARY'S OWN definitions; the reference has no simulator.
//
// One PP_HD function, sense_scene, behind the kernel (k_sense) and the host twin. It uses only
// + - * /, IEEE sqrt and integer arithmetic, and both sides are compiled with -ffp-contract=off, so
// device and host agree bit for bit. The truth (the telemetry k_sim leaves) is only read; the sensed
// rows go to the sensor state's own arrays.
//
// Per truth row r (id j, centre c) of a scene with ego e, a = c - e, carried frame number f and
// global scene gs, in this order:
//   occlusion  (occlusion_radius > 0 only) some truth row k != r with b = c_k - e has b.b < a.a and
//              |b - u a|^2 <= occlusion_radius^2, u = (a.b) / (a.a) clamped to [0, 1]:
//              the sight line's segment e..c passes within the radius of a nearer car's centre
//   dropout    (not occluded) (double)w 2^-32 < dropout_prob, w = word 0 of block q = 4
//   noise      (reported) sp = pos_sigma + pos_sigma_per_m sqrt(a.a); x + sp g0, y + sp g1,
//              vx + vel_sigma g2, vy + vel_sigma g3; a field whose sigma is exactly 0 is copied (sp
//              counts as 0 where both its coefficients are 0, whatever a.a: also at infinity or NaN)
// Philox4x32-10 blocks: key = seed, counter = {gs lo, gs hi, (f PP_NOISE_CAR_STRIDE + (uint32)j) 8 + q,
// kTag} (mod 2^32); g_q = ppsynth::ih_unit of block q = 0..3. A car's draws depend on (seed, gs, f, j)
// only: not on its row, the other cars or the sharding. Blocks nobody reads are not computed.
// The occlusion test is O(rows^2) per scene.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "pp_synth.h"

namespace ppsensor {

constexpr uint32_t kTag = 0x53454E53u;     // the stream's fourth counter word ("SENS")
constexpr int kDropBlock = 4;              // q of the dropout block

// pp_sensor_cfg_default's values (host only): the identity sensor
inline void cfg_default(pp_sensor_cfg* c) {
    memset(c, 0, sizeof(*c));
    c->seed = 0x5EED0003ull;
}

// finite and >= 0 (x - x is NaN for an infinity)
PP_HD inline bool amount_ok(double x) { return x >= 0 && x - x == 0; }
PP_HD inline bool cfg_ok(const pp_sensor_cfg& c) {
    return c.first_scene >= 0 && amount_ok(c.pos_sigma) && amount_ok(c.pos_sigma_per_m) && amount_ok(c.vel_sigma) &&
           amount_ok(c.occlusion_radius) && c.dropout_prob >= 0 && c.dropout_prob <= 1;
}

// third counter word of block q of car `car` in frame `frame` (mod 2^32)
PP_HD inline uint32_t block_of(uint32_t frame, uint32_t car, int q) {
    return (frame * (uint32_t)PP_NOISE_CAR_STRIDE + car) * 8u + (uint32_t)q;
}

// one block (pp_sensor_gauss, pp_sensor_word)
PP_HD inline void block(uint64_t seed, uint64_t gs, uint32_t frame, uint32_t car, int q, uint32_t out[4]) {
    ppsynth::philox4x32(seed, gs, block_of(frame, car, q), out, kTag);
}

// blocks q = 0..3 of one car at once, their rounds interleaved (independent chains), as
// ppsynth::mc_gauss4 does
PP_HD inline void gauss4(uint64_t seed, uint64_t gs, uint32_t frame, uint32_t car, double g[4]) {
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t ctr[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        ctr[q][0] = (uint32_t)gs; ctr[q][1] = (uint32_t)(gs >> 32);
        ctr[q][2] = block_of(frame, car, q); ctr[q][3] = kTag;
    }
#pragma unroll
    for (int r = 0; r < 10; r++) {
#pragma unroll
        for (int q = 0; q < 4; q++) ppsynth::philox_round(ctr[q], key);
        key[0] += 0x9E3779B9u;
        key[1] += 0xBB67AE85u;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) g[q] = ppsynth::ih_unit(ctr[q]);
}

// The truth of a batch as the sensor reads it (pointers into the telemetry's arrays).
struct Truth {
    int64_t S;
    int stride;                    // car_stride: rows every [r * S + s] array holds
    const double *ego_x, *ego_y;
    const int32_t *n_cars, *car_id;
    const double *car_x, *car_y, *car_vx, *car_vy;
};

// Scene s of the batch: fills the state's sensed rows, count and fates, and advances its frame.
PP_HD inline void sense_scene(const Truth& T, int64_t s, const pp_sensor_cfg& cfg, const pp_sensor& st) {
    const int64_t S = T.S;
    int n = T.n_cars[s];
    n = n < 0 ? 0 : (n > T.stride ? T.stride : n);
    const double ex = T.ego_x[s], ey = T.ego_y[s];
    const uint32_t f = (uint32_t)st.frame[s];
    const uint64_t gs = (uint64_t)(cfg.first_scene + s);
    const double R2 = cfg.occlusion_radius * cfg.occlusion_radius;
    const bool noisy_p = cfg.pos_sigma != 0 || cfg.pos_sigma_per_m != 0, noisy_v = cfg.vel_sigma != 0;
    int out = 0;
    for (int r = 0; r < n; r++) {
        const int64_t ix = (int64_t)r * S + s;
        const int32_t id = T.car_id[ix];
        const double cx = T.car_x[ix], cy = T.car_y[ix];
        const double ax = cx - ex, ay = cy - ey;
        const double aa = ax * ax + ay * ay;
        bool hidden = false;
        if (cfg.occlusion_radius > 0) {
            for (int k = 0; k < n; k++) {
                if (k == r) continue;
                const int64_t kx = (int64_t)k * S + s;
                const double bx = T.car_x[kx] - ex, by = T.car_y[kx] - ey;
                const double bb = bx * bx + by * by;
                if (!(bb < aa)) continue;                     // (aa > bb >= 0: the division is safe)
                double u = (ax * bx + ay * by) / aa;
                u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
                const double dx = bx - u * ax, dy = by - u * ay;
                if (dx * dx + dy * dy <= R2) hidden = true;
            }
        }
        int32_t fate = PP_SENSE_REPORTED;
        if (hidden) {
            fate = PP_SENSE_OCCLUDED;
        } else if (cfg.dropout_prob > 0) {
            uint32_t w[4];
            block(cfg.seed, gs, f, (uint32_t)id, kDropBlock, w);
            if ((double)w[0] * 0x1p-32 < cfg.dropout_prob) fate = PP_SENSE_DROPPED;
        }
        st.fate[ix] = fate;
        if (fate != PP_SENSE_REPORTED) continue;
        double x = cx, y = cy, vx = T.car_vx[ix], vy = T.car_vy[ix];
        const double sp = noisy_p ? cfg.pos_sigma + cfg.pos_sigma_per_m * sqrt(aa) : 0.0;
        if (sp != 0 || noisy_v) {
            double g[4];
            gauss4(cfg.seed, gs, f, (uint32_t)id, g);
            if (sp != 0) { x = x + sp * g[0]; y = y + sp * g[1]; }
            if (noisy_v) { vx = vx + cfg.vel_sigma * g[2]; vy = vy + cfg.vel_sigma * g[3]; }
        }
        const int64_t ox = (int64_t)out * S + s;
        st.car_id[ox] = id;
        st.car_x[ox] = x; st.car_y[ox] = y;
        st.car_vx[ox] = vx; st.car_vy[ox] = vy;
        out++;
    }
    for (int r = n; r < T.stride; r++) st.fate[(int64_t)r * S + s] = PP_SENSE_NONE;
    st.n_cars[s] = out;
    st.frame[s] = (int32_t)(f + 1u);
}

}  // namespace ppsensor
