// pp_k_frame.h — device: what every stage shares. The map view, the streaming accesses, the output
// frame and its turns (TrajectoryBuilder::build's local -> global transform, src/main.cpp:786-823,
// 978-1007, 1033-1037), the tuning constants, the winner record, the map's staging into LDS and a
// car's velocity (src/main.cpp:1343-1346). Part of pp_eval.hip's translation unit.
#pragma once

// kMapArrays arrays of n: ref_x ref_y nx ny lc_x[NL] lc_y[NL] llen[NL] lden[NL] lrcp[NL]
// atab: the approach table (global memory; build_atab; null: none); atab_lds: it fits k_prep<true,
// false>'s LDS after the map (that kernel stages it there: the host passes it only then)
struct MapG { const double* buf; int n; int fastm; WGrid wg; const double2* wseg; const double* atab; int atab_lds; };

// |angle| bound for the hot loop: the loop adds at most 2*pi per curvature adjustment over
// <= PP_MAX_POINTS steps, which keeps every sin/cos argument below ppm::kMediumMax.
constexpr double kSlowAngle = 1.0e5;
constexpr int kLimSlow = 1 << 7;   // internal bit in PrepV.lim_mask
static_assert(NL <= 6, "lim_mask: bit 0 in-lane limit, bits 1..NL lane limits, bit 7 kLimSlow");

__device__ __forceinline__ MapV map_view(const double* b, int n, int fastm = 0) {
    MapV m;
    m.ref_x = b; m.ref_y = b + n; m.nx = b + 2 * n; m.ny = b + 3 * n;
    m.lc_x = b + 4 * n; m.lc_y = b + (4 + NL) * n; m.llen = b + (4 + 2 * NL) * n;
    m.lden = b + (4 + 3 * NL) * n; m.lrcp = b + (4 + 4 * NL) * n; m.n = n; m.fastm = fastm;
    return m;
}

// The winner record (written once by k_cand, read once by k_emit), next_x/next_y (written once)
// and every emitted path point are nontemporal (streaming) accesses
#define PP_ST(p, v) __builtin_nontemporal_store((v), (p))
#define PP_LD(p) __builtin_nontemporal_load(p)
// one (x, y) path point: a 16-B store (p 16-B aligned: paths are [.., c] pairs of doubles)
__device__ __forceinline__ void st_xy(double* p, double x, double y) {
    typedef double dv2 __attribute__((ext_vector_type(2)));
    const dv2 xy = {x, y};
    __builtin_nontemporal_store(xy, (dv2*)p);
}
// ---- The output frame: the local -> global transform of TrajectoryBuilder::build (src/main.cpp:
// 786-823, 994-1007, 1033-1037). No decision of the loop reads it, so its turns (curvature
// adjustments) are evaluated in fused multiply-adds with an angle-sum rotation of the heading; every
// launch shape that writes the reference decision's next_x/next_y (k_emit, the fused small-batch
// kernels) or a winner's (k_winner) calls these same functions, so their outputs stay bit-identical
// to each other (and within ~1e-11 m of the reference after a turn, equal to it before the first
// one). k_cand's all-paths mode has a cheaper variant below (frame_step, turn_narrow).
struct OutFrame { double cx, cy, ca, sa; };   // centre, cos and sin of the frame's heading
// a point: the reference's own operations (src/main.cpp:1033-1036), unfused: until a path's first
// curvature adjustment its points carry the reference's bits, and in a closed loop those first
// points are the next frame's previous path (its ego speed, heading and spline knots)
__device__ __forceinline__ void frame_pt(const OutFrame& f, double px, double py, double& ox, double& oy) {
    ox = (px * f.ca - py * f.sa) + f.cx;
    oy = (px * f.sa + py * f.ca) + f.cy;
}
// the turn of a curvature adjustment (src/main.cpp:986-997) at local point (px, py): the centre
// rotates about the current output point, the heading's (cos, sin) by the angle-sum rotation
__device__ __forceinline__ void frame_turn(OutFrame& f, double px, double py, double cr, double sr) {
    double tx, ty;
    frame_pt(f, px, py, tx, ty);
    const double vx = f.cx - tx, vy = f.cy - ty;
    f.cx = tx + __builtin_fma(vx, cr, -(vy * sr));
    f.cy = ty + __builtin_fma(vx, sr, vy * cr);
    const double nca = __builtin_fma(f.ca, cr, -(f.sa * sr)), nsa = __builtin_fma(f.sa, cr, f.ca * sr);
    f.ca = nca;
    f.sa = nsa;
}
// the turn angle rot = nad - adiff (src/main.cpp:978-986), nad = +-nc / speed / 50 with the sign of
// adiff: k_cand<false> (speed +0 or in [2^-113, 2^21]) by a reciprocal, the checked instantiation by
// IEEE divisions (speed 0: +-inf or NaN, which turns the rest of the path into NaN either way)
template <bool kLarge>
__device__ __forceinline__ double turn_angle(double nc, double speed, double adiff) {
    double nad = kLarge ? nc / speed / 50 : (nc * 0.02) * ppm::rcp_nr(speed);
    if (adiff < 0) nad *= -1;
    return nad - adiff;
}
// sin and cos of a turn: fdlibm's kernel polynomials in fused form on [-pi/4, pi/4] (< 1 ulp,
// tests/test_math_primitives.py; cos keeps the rounding error of 1 - z/2 as fdlibm's does: without
// it 1.19 ulp); a
// wider turn (rare: a wide step turn, or a step slower than ~0.7 m/s) is first reduced by the
// nearest multiple of pi/2 (two-part Cody-Waite: |error| < 1e-15 rad up to kMediumMax, plenty for an
// output frame) and its quadrant applied after; beyond kMediumMax (only from an absurd telemetry
// heading, in the checked instantiation) the library's reduction
// a constant materialised at its use (scalar moves) rather than hoisted out of the step loop into
// registers that the loop then holds throughout
__device__ __forceinline__ double kc(double v) {
    asm volatile("" : "+s"(v));
    return v;
}
template <bool kLarge>
__device__ __forceinline__ void turn_sincos(double r, double& s, double& c) {
    double y = r;
    int q = 0;
    if (__builtin_expect(!(fabs(r) <= 0.78539816339744828), 0)) {
        if (kLarge && !(fabs(r) <= ppm::kMediumMax)) {
            ppm::sincos_pp<true>(r, s, c);
            return;
        }
        const double k = __builtin_rint(r * 6.36619772367581382433e-01);
        y = __builtin_fma(-k, kc(1.57079632673412561417e+00), r);
        y = __builtin_fma(-k, kc(6.07710050650619224932e-11), y);
        q = (int)k;
    }
    const double z = y * y;
    double ps = __builtin_fma(z, kc(1.58969099521155010221e-10), kc(-2.50507602534068634195e-08));
    ps = __builtin_fma(z, ps, kc(2.75573137070700676789e-06));
    ps = __builtin_fma(z, ps, kc(-1.98412698298579493134e-04));
    ps = __builtin_fma(z, ps, kc(8.33333333332248946124e-03));
    ps = __builtin_fma(z, ps, kc(-1.66666666666666324348e-01));
    double pc = __builtin_fma(z, kc(-1.13596475577881948265e-11), kc(2.08757232129817482790e-09));
    pc = __builtin_fma(z, pc, kc(-2.75573143513906633035e-07));
    pc = __builtin_fma(z, pc, kc(2.48015872894767294178e-05));
    pc = __builtin_fma(z, pc, kc(-1.38888888888741095749e-03));
    pc = __builtin_fma(z, pc, kc(4.16666666666666019037e-02));
    s = __builtin_fma(y * z, ps, y);
    // 1 - z/2 rounds: its error (1 - w) - hz is exact and joins the small term, as in fdlibm's kernel
    const double hz = 0.5 * z, w = 1.0 - hz;
    c = w + __builtin_fma(z * z, pc, (1.0 - w) - hz);
    if (__builtin_expect(q != 0, 0)) {
        if (q & 1) { const double t = s; s = c; c = -t; }
        if (q & 2) { s = -s; c = -c; }
    }
}

// k_cand's all-paths mode (output mode 4): the same output frame, cheaper. Every candidate writes
// its path there, so the point transform runs on every lane-step and a turn on about half of all
// wave-steps (for one lane in ten); the turn angle's reciprocal takes one Newton step. The paths'
// tolerance is 1e-6 m, and no decision and no closed loop reads these points (the reference
// decision's next_x/next_y and every fed-back path come from frame_turn / k_emit).
__device__ __forceinline__ double turn_angle_fast(double nc, double speed, double adiff) {
    double r = __builtin_amdgcn_rcp(speed);
    r = __builtin_fma(__builtin_fma(-speed, r, 1.0), r, r);
    double nad = (nc * 0.02) * r;          // (speed, hence nad, may be negative)
    if (adiff < 0) nad = -nad;
    return nad - adiff;
}
// Round 5: k_cand's all-paths frame without a centre. The reference's turn rotates the centre
// about the current output point tp (src/main.cpp:995-1004), so tp stays where it is and every
// later point is o_{k+1} = o_k + R_{k+1} (p_{k+1} - p_k): the loop keeps the last output point o
// and the heading (ca, sa) only, and a point is o plus the rotated local step (frame_step: two
// fused multiply-adds per coordinate). A narrow turn (the step's angle came from asin(u_prev x u):
// |adiff| <= 0.0709) rotates by rot = nad - adiff, i.e. by R(nad) R(-adiff), and (cos, sin)(adiff)
// are the step's own unit-vector products (dt, cr): only sin/cos of |nad| < |adiff| are left,
// short Taylor polynomials (sincos_small). The points differ
// from the reference's by rounding only (the summed steps: ~1e-13 m over a 100-point path); no
// decision reads them.
// a narrow step turn (asin_small's domain): u_prev . u > 0 and |u_prev x u| <= kStepSinMax
#define PP_NARROW(dt, cr) ((dt) > 0 && fabs(cr) <= ppm::kStepSinMax)
__device__ __forceinline__ void frame_step(double ca, double sa, double dpx, double dpy, double& ox, double& oy) {
    ox = __builtin_fma(dpx, ca, __builtin_fma(-dpy, sa, ox));
    oy = __builtin_fma(dpx, sa, __builtin_fma(dpy, ca, oy));
}
// sin and cos of |x| <= 0.0709: sin through x^7 (next term x^9/9! < 1.3e-16), cos through x^8 (next
// term x^10/10! < 1e-18)
__device__ __forceinline__ void sincos_small(double x, double& s, double& c) {
    const double z = x * x;
    double ps = __builtin_fma(z, kc(-1.98412698412698412698e-04), kc(8.33333333333333333333e-03));
    ps = __builtin_fma(z, ps, kc(-1.66666666666666666667e-01));
    s = __builtin_fma(x * z, ps, x);
    double pc = __builtin_fma(z, kc(2.48015873015873015873e-05), kc(-1.38888888888888888889e-03));
    pc = __builtin_fma(z, pc, kc(4.16666666666666666667e-02));
    pc = __builtin_fma(z, pc, -0.5);
    c = __builtin_fma(z, pc, 1.0);
}
// the heading turned by (cr, sr) = (cos, sin) of the rotation
__device__ __forceinline__ void frame_rot(double& ca, double& sa, double cr, double sr) {
    const double nca = __builtin_fma(ca, cr, -(sa * sr)), nsa = __builtin_fma(sa, cr, ca * sr);
    ca = nca;
    sa = nsa;
}
// a narrow turn: nad = +-nc / speed / 50 with adiff's sign (src/main.cpp:983-984; adiff is never
// -0: x - pi rounds an exact cancellation to +0), (cos, sin)(rot) = R(nad) applied to (dt, -cr)
__device__ __forceinline__ void turn_narrow(double& ca, double& sa, double nc, double speed, double adiff,
                                            double dt, double cr) {
    double r = __builtin_amdgcn_rcp(speed);
    r = __builtin_fma(__builtin_fma(-speed, r, 1.0), r, r);
    const double nad = __builtin_copysign((nc * 0.02) * r, adiff);
    double sn, cn;
    sincos_small(nad, sn, cn);
    frame_rot(ca, sa, __builtin_fma(cn, dt, sn * cr), __builtin_fma(sn, dt, -(cn * cr)));
}
// Tuning constants (each measured against its alternatives):
constexpr int kEmitChunk = 4;      // emit_scene_pre (small batches): recorded steps loaded together per lane
constexpr int kEmitRows = 8;       // k_emit (large batches, emit_scene_rows): output rows per load round
constexpr int kWalkPf = 4;         // segments of the control-point walk loaded ahead (get_lane_pos_fwd)
constexpr int kPrepWaves = 3;      // k_prep waves per SIMD (kW4: 4)
constexpr int kCandWaves = 4;      // k_cand waves per SIMD (<= 128 VGPRs), every instantiation
// Winner record (k_cand -> k_emit), room = N - K steps of scene s, rstride = room S: point-major
// arrays, pos_x at rec[g S + s], pos_y at rec[rstride + g S + s], the rotation of an adjusted step
// at rec[2 rstride + g S + s] (every address of scene s is = s mod S: a wave's accesses coalesce)
__device__ __forceinline__ double* rec_px(double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s) {
    (void)rstride;
    return rec + g * S + s;
}
__device__ __forceinline__ double* rec_py(double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s) {
    return rec + rstride + g * S + s;
}
__device__ __forceinline__ double* rec_rot(double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s) {
    return rec + 2 * rstride + g * S + s;
}
__device__ __forceinline__ const double* rec_rot(const double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s) {
    return rec_rot((double*)rec, rstride, g, S, s);
}
__device__ __forceinline__ void rec_st(double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s,
                                       double x, double y) {
    PP_ST(rec_px(rec, rstride, g, S, s), x);
    PP_ST(rec_py(rec, rstride, g, S, s), y);
}
__device__ __forceinline__ void rec_ld(const double* rec, int64_t rstride, int64_t g, int64_t S, int64_t s,
                                       double& x, double& y) {
    double* r = (double*)rec;
    x = PP_LD(rec_px(r, rstride, g, S, s));
    y = PP_LD(rec_py(r, rstride, g, S, s));
}
// The map into LDS (16-B aligned both sides): 16-B loads, each thread's loads issued before its LDS
// stores, so a block stages a map of up to 8 x 512 doubles (highway_map.csv: 3,439) in one round
// trip to memory instead of one per element (the single-frame kernel waits for it)
__device__ __forceinline__ void stage_map(double* __restrict__ dst, const double* __restrict__ src, int nd) {
    typedef double dv2 __attribute__((ext_vector_type(2)));
    constexpr int kU = 8;
    const int n2 = nd / 2;
    for (int i0 = threadIdx.x; i0 < n2; i0 += kU * blockDim.x) {
        dv2 v[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n2) v[u] = ((const dv2*)src)[i];
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < n2) ((dv2*)dst)[i] = v[u];
        }
    }
    if ((nd & 1) && threadIdx.x == 0) dst[nd - 1] = src[nd - 1];
}
// kLdsMap: the map (kMapArrays n doubles) is staged in LDS (n <= kLdsMapMax: <= 62.4 KB, 600
// waypoints at three lanes); larger maps are read from global memory (L2-resident) by the same code.
constexpr int kLdsMapMax = 62400 / (8 * kMapArrays);

// the velocity k_prep's car pass used for the car of iteration index it (src/main.cpp:1343-1346):
// the table slot it (written or stale) with a car table, else row it plus its Monte-Carlo noise
__device__ __forceinline__ void car_velocity(const pp_scene_batch& in, const pp_params& P, int64_t S,
                                             int64_t s, int draw, bool tab, int it, double& vx, double& vy) {
    const int64_t ix = (int64_t)it * S + s;
    if (tab) { vx = in.tab_vx[ix]; vy = in.tab_vy[ix]; return; }
    vx = in.car_vx[ix]; vy = in.car_vy[ix];
    if (draw > 0) {
        const uint64_t gs = (uint64_t)(P.noise_first_scene + s);
        vx += P.noise_vel_sigma * ppsynth::mc_gauss(P.noise_seed, gs, draw, it, 2);
        vy += P.noise_vel_sigma * ppsynth::mc_gauss(P.noise_seed, gs, draw, it, 3);
    }
}
