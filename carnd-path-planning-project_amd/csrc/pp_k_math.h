// pp_k_math.h — device: k_math, the candidate loop's FP64 primitives evaluated over arrays
// (pp_math_eval, include/pp.h PP_MATH_*). One lane per element; each kind calls the function the
// loop calls (ppm:: of pp_math.h, the SpeedController wrappers of pp_device.h, the turn functions of
// pp_k_frame.h), never a restatement of it, so tests/test_math_primitives.py holds each one's
// written accuracy claim on the code the planner runs. Part of pp_eval.hip's translation unit;
// nothing here depends on NL.
#pragma once

// inputs and outputs per kind (pp_math_eval's argument check and the kernel's loads)
struct MathArity { int nin, nout; };
__host__ __device__ inline MathArity math_arity(int kind) {
    switch (kind) {
        case PP_MATH_SINCOS: case PP_MATH_SINCOS_NOLARGE: case PP_MATH_TURN_SINCOS:
        case PP_MATH_TURN_SINCOS_NOLARGE: case PP_MATH_SINCOS_SMALL: return {1, 2};
        case PP_MATH_ATAN2_PP: case PP_MATH_ATAN2_FAST: case PP_MATH_ATAN2_UNIT:
        case PP_MATH_DIV_RCP_AUTO: case PP_MATH_DIV_RCP_NC_AUTO: case PP_MATH_DIV_RCP_N:
        case PP_MATH_DIV_RCP_D: return {2, 1};
        case PP_MATH_ASIN_SMALL: case PP_MATH_RCP_NR: case PP_MATH_DIV50: case PP_MATH_DIV50_NC:
        case PP_MATH_FMOD_2PI: case PP_MATH_FMOD_2PI_SMALL: case PP_MATH_SPEED_IN_RANGE: return {1, 1};
        case PP_MATH_DIV_RCP: case PP_MATH_DIV_RCP_NC: case PP_MATH_TURN_ANGLE:
        case PP_MATH_TURN_ANGLE_NOLARGE: case PP_MATH_TURN_ANGLE_FAST: return {3, 1};
        case PP_MATH_SQRT_RD: return {1, 3};
        case PP_MATH_SC_SPEED: case PP_MATH_SC_SPEED_R: case PP_MATH_SC_SPEED_R_NC:
        case PP_MATH_SC_OVERRIDE: case PP_MATH_SC_OVERRIDE_R: case PP_MATH_SC_OVERRIDE_R_NC: return {4, 1};
        default: return {0, 0};
    }
}

__global__ __launch_bounds__(256) void k_math(int kind, const double* a, const double* b, const double* c,
                                              const double* d, double* out0, double* out1, double* out2,
                                              int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MathArity ar = math_arity(kind);
    const double va = a[i];
    const double vb = ar.nin > 1 ? b[i] : 0.0, vc = ar.nin > 2 ? c[i] : 0.0;
    double r0 = __builtin_nan(""), r1 = r0, r2 = r0;
    switch (kind) {
        case PP_MATH_SINCOS: ppm::sincos_pp<true>(va, r0, r1); break;
        case PP_MATH_SINCOS_NOLARGE: ppm::sincos_pp<false>(va, r0, r1); break;
        case PP_MATH_ATAN2_PP: r0 = ppm::atan2_pp(va, vb); break;
        case PP_MATH_ATAN2_FAST: r0 = ppm::atan2_fast(va, vb); break;
        case PP_MATH_ATAN2_UNIT: r0 = ppm::atan2_unit(va, vb); break;
        case PP_MATH_ASIN_SMALL: r0 = ppm::asin_small(va); break;
        case PP_MATH_RCP_NR: r0 = ppm::rcp_nr(va); break;
        case PP_MATH_DIV_RCP: r0 = ppm::div_rcp(va, vb, vc); break;
        case PP_MATH_DIV_RCP_NC: r0 = ppm::div_rcp_nc(va, vb, vc); break;
        case PP_MATH_DIV_RCP_AUTO: r0 = ppm::div_rcp(va, vb, ppm::rcp_nr(vb)); break;
        case PP_MATH_DIV_RCP_NC_AUTO: r0 = ppm::div_rcp_nc(va, vb, ppm::rcp_nr(vb)); break;
        case PP_MATH_DIV50: r0 = ppm::div_rcp(va, 50.0, 0.02); break;
        case PP_MATH_DIV50_NC: r0 = ppm::div50_nc(va); break;
        case PP_MATH_SQRT_RD: {
            const bool dok = ppm::sqrt_rd(va, r0, r1);
            r2 = dok ? 1.0 : 0.0;
            break;
        }
        case PP_MATH_DIV_RCP_N: case PP_MATH_DIV_RCP_D: {      // as run_candidate's step: sqrt_rd first
            double dd, rd;
            const bool dok = ppm::sqrt_rd(vb, dd, rd);
            r0 = kind == PP_MATH_DIV_RCP_N ? ppm::div_rcp_n(va, dd, rd, dok) : ppm::div_rcp_d(va, dd, rd, dok);
            break;
        }
        case PP_MATH_FMOD_2PI: r0 = ppm::fmod_2pi(va); break;
        case PP_MATH_FMOD_2PI_SMALL: r0 = ppm::fmod_2pi_small(va); break;
        case PP_MATH_TURN_SINCOS: turn_sincos<true>(va, r0, r1); break;
        case PP_MATH_TURN_SINCOS_NOLARGE: turn_sincos<false>(va, r0, r1); break;
        case PP_MATH_SINCOS_SMALL: sincos_small(va, r0, r1); break;
        case PP_MATH_TURN_ANGLE: r0 = turn_angle<true>(va, vb, vc); break;
        case PP_MATH_TURN_ANGLE_NOLARGE: r0 = turn_angle<false>(va, vb, vc); break;
        case PP_MATH_TURN_ANGLE_FAST: r0 = turn_angle_fast(va, vb, vc); break;
        case PP_MATH_SC_SPEED: case PP_MATH_SC_SPEED_R: case PP_MATH_SC_SPEED_R_NC: {
            // d: planes of n — shift, then the step count k (t = 0.02 k)
            const SC sc = {va, vb, vc, d[i]};
            const double t = 0.02 * d[n + i];
            if (kind == PP_MATH_SC_SPEED) r0 = sc_get_speed(sc, t);
            else if (kind == PP_MATH_SC_SPEED_R) r0 = sc_get_speed_r<true>(sc, t, ppm::rcp_nr(sc.ttime));
            else r0 = sc_get_speed_r<false>(sc, t, ppm::rcp_nr(sc.ttime));
            break;
        }
        case PP_MATH_SC_OVERRIDE: case PP_MATH_SC_OVERRIDE_R: case PP_MATH_SC_OVERRIDE_R_NC: {
            // d: planes of n — shift, the step count k (t = 0.02 k), the overriding speed
            SC sc = {va, vb, vc, d[i]};
            const double t = 0.02 * d[n + i], speed = d[2 * n + i];
            if (kind == PP_MATH_SC_OVERRIDE) sc_override(sc, t, speed);
            else if (kind == PP_MATH_SC_OVERRIDE_R) sc_override_r<true>(sc, t, speed, ppm::rcp_nr(sc.target - sc.start));
            else sc_override_r<false>(sc, t, speed, ppm::rcp_nr(sc.target - sc.start));
            r0 = sc.shift;
            break;
        }
        case PP_MATH_SPEED_IN_RANGE: r0 = speed_in_range(va) ? 1.0 : 0.0; break;
        default: break;
    }
    out0[i] = r0;
    if (ar.nout > 1) out1[i] = r1;
    if (ar.nout > 2) out2[i] = r2;
}
