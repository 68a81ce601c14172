// pp_k_cand.h — device: K2, the candidates. run_candidate (the 0.02 s resampling loop with the
// accel/curvature limiter, src/main.cpp:905-1041), the candidate cost, the replay of a winner's path
// inside a block (emit_scene_pre), cand_group (one group of the candidate grid by a workgroup) and
// k_cand. Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// Phase B: the resampling loop of one candidate (src/main.cpp:845-1041)
// ------------------------------------------------------------------------------------------------
// adj0/adj1: the adjusted steps 0-63 / 64-127 (two registers: an indexed pair would live in scratch)
struct CandRes { double acc_sum, travelled; int ng; uint32_t flags; uint64_t adj0, adj1; };

// Output modes. The curvature adjustment (src/main.cpp:972-1018) rotates only the local->global
// transform (centre, angle); the local path (pos_x, pos_y, arg, speed, angles) that the cost reads
// never depends on it, so a cost-only lane skips the transform, its sin/cos and the stores.
//   kOutMode 0: cost only;  2: every lane produces points;  4: the same with k_cand's cheaper
//   output frame (frame_step, turn_narrow);  3: lanes with out_on RECORD their local path (pos after each step, rotation angle of each
//   curvature adjustment + a bitmask of the adjusted steps) for k_emit, which replays the
//   transform — the expensive sin/cos of the adjustments leaves the candidate loop entirely.
// Point g goes to wx[g*ws], wy[g*ws] (if wx) and px[g*ps], px[g*ps+1] (if px); in mode 3 the record
// goes to rec[g*ws] (pos_x), rec[(RN + g)*ws] (pos_y), rec[(2 RN + g)*ws] (rotation), RN = room.
// The current spline segment (bounds + coefficients) stays in registers; the segment changes every
// ~10-40 steps, so most steps read no slot memory.
template <bool kLarge, int kOutMode>
__device__ CandRes run_candidate(const pp_params& P, const Slot& sl, double cx, double cy,
                                 double angle, double ca0, double sa0, SC sc, int room, double* wx,
                                 double* wy, int64_t ws, double* px, int64_t ps, bool out_on = true,
                                 double* rec = nullptr, int dcls = 0, int64_t rs = 0) {
    (void)dcls;   // PP_DIAG builds: candidate class (|L - ego lane|) for the census
    // kOutMode 3: rec = the record base + rs (the scene), ws = the batch's scene count (rec_st)
    const bool kOut = kOutMode == 2 || kOutMode == 4;
    const bool kRec = kOutMode == 3 && out_on;
    const int64_t rstride = (int64_t)room * ws;
    CandRes R;
    R.acc_sum = 0; R.travelled = 0; R.ng = 0; R.flags = 0; R.adj0 = 0; R.adj1 = 0;
    const int nk = sl.m(0), ncp = sl.m(1), npk = sl.m(2), mflags = sl.m(3);
    if (mflags & kMetaTrunc) R.flags |= PP_ST_SPLINE_TRUNC;
    if (mflags & kMetaWalkFail) R.flags |= PP_ST_NAN;
    double pos_x = 0, pos_y = 0;
    OutFrame F = {cx, cy, ca0, sa0};
    double opx = cx, opy = cy;        // mode 4: the last output point (the frame's image of (0, 0))
    (void)angle;      // the frame turns by rotating (ca, sa) (src/main.cpp:996-997)
    double cur_t = 0.02;
    int ng = 0;
    if (mflags & kMetaFallback) {                                       // :848-901
        R.flags |= PP_ST_FALLBACK;
        const double speed = sc_get_speed(sc, cur_t);
        double cang = 0;
        int nc = 1;
        while (ng < room && nc < ncp) {
            const double dstep = speed / 50;
            const double ndx = sl.x(npk + nc) - pos_x, ndy = sl.y(npk + nc) - pos_y;
            const double cpd = sqrt(ndx * ndx + ndy * ndy);
            if (cpd < 5) { nc++; continue; }
            cur_t += 0.02;
            const double nca = ppm::atan2_fast(ndy, ndx);
            const double adiff = ppm::fmod_2pi(nca - cang + 3 * kPi) - kPi;
            const double min_radius = s_max(10.0, speed * speed / 4);
            const double rps = speed / min_radius;
            const double mas = rps / 50;
            if (fabs(adiff) > mas) {
                if (adiff > 0) cang += mas; else cang -= mas;
            } else {
                cang += adiff;
            }
            double sc_, cc_;
            ppm::sincos_pp<kLarge>(cang, sc_, cc_);
            pos_x += cc_ * dstep;
            pos_y += sc_ * dstep;
            if (kOutMode != 0 && kOut) {
                double ox, oy;
                frame_pt(F, pos_x, pos_y, ox, oy);
                if (wx && PP_CHKP(wx + ng * ws, nx, nnext, 1) && PP_CHKP(wy + ng * ws, ny, nnext, 2)) { wx[ng * ws] = ox; wy[ng * ws] = oy; }
                if (px && PP_CHKP(px + ng * ps, paths, npaths, 3) && PP_CHKP(px + ng * ps + 1, paths, npaths, 3)) st_xy(px + ng * ps, ox, oy);
            }
            if (kOutMode == 3 && kRec && PP_CHKP(rec_px(rec - rs, rstride, ng, ws, rs), rec, nrec, 4) && PP_CHKP(rec_py(rec - rs, rstride, ng, ws, rs), rec, nrec, 5)) rec_st(rec - rs, rstride, ng, ws, rs, pos_x, pos_y);
            ng++;
            R.travelled += dstep;
        }
        R.ng = ng;
        return R;
    }
    // cached segment: valid while seg_lo < x <= seg_hi (NaN x never valid)
    int cnt = -1;                    // #knots with X < x (std::lower_bound position); -1: none yet
    double seg_lo = 1.0, seg_hi = -__builtin_inf(), sx = 0, sa_ = 0, sb = 0, sc_ = 0, sy = 0;
    double arg = 0, prev_speed = sc.start;
    double uxp = 1.0, uyp = 0.0;     // previous step direction (angle 0: the local frame's x axis)
    // 1 / (target - start) for SpeedController::override_speed (constant over the walk)
    const double rds = ppm::rcp_nr(sc.target - sc.start);
    double rtt = ppm::rcp_nr(sc.ttime);
    PP_DIAGC(20, true);     // (waves entering the loop)
#ifdef PP_LIMCENSUS
    double ref_pa = 0;      // the reference's prev_angle (src/main.cpp:906): the previous step's atan2
#endif
    // the divisions by 50 and by the ramp time: reciprocal + correction (k_cand<false>: unchecked)
#define PP_DIV50(v) (kLarge ? ppm::div_rcp(v, 50.0, 0.02) : ppm::div50_nc(v))
    // one step of the loop (src/main.cpp:911-1040): (uxp, uyp) the previous step's unit direction,
    // prev_speed its speed; the step's own go to (uxn, uyn, psn). The loop runs two steps per
    // iteration with the two register sets alternating (no copies at the back edge)
    auto step = [&](const double uxp, const double uyp, const double prev_speed, double& uxn, double& uyn,
                    double& psn) __attribute__((always_inline)) {
            PP_REGION("head");
            PP_DIAGC(0, true);
            PP_DIAGC(2, !(s_max(cur_t - sc.shift, 0.0) > sc.ttime));
            double speed = sc_get_speed_r<kLarge>(sc, cur_t, rtt);
            double dstep = PP_DIV50(speed);
            const double x = arg + dstep;
            // tk::spline::operator() (spline.h:375-396)
            if (!(seg_lo < x && x <= seg_hi)) {
                PP_REGION("seg");
                // forward miss (x passed the cached segment's end; the first step starts from cnt = -1,
                // seg_hi = -inf): x(cnt) = seg_hi < x is known, so the walk resumes one knot further
                // and the bounds come from the walk's own reads — one LDS round trip for the knot and
                // one for the coefficients, instead of the two loops' re-reads
                if (__builtin_expect(x > seg_hi, 1)) {
                    double xlo = seg_hi, xhi;
                    cnt++;
                    for (;;) {
                        xhi = cnt < nk ? sl.x(cnt) : __builtin_inf();
                        if (!(xhi < x)) break;
                        xlo = xhi;
                        cnt++;
                    }
                    seg_lo = xlo;
                    seg_hi = xhi;
                    const int idx = cnt - 1 > 0 ? cnt - 1 : 0;
                    sx = cnt > 0 ? xlo : xhi;
                    sa_ = cnt == 0 ? 0.0 : sl.a(idx); sb = sl.b(idx); sc_ = sl.c(idx); sy = sl.y(idx);
                } else {
                    PP_REGION("segback");
                    PP_DIAGC(21, true);
                    if (cnt < 0) cnt = 0;
                    while (cnt < nk && sl.x(cnt) < x) cnt++;
                    while (cnt > 0 && !(sl.x(cnt - 1) < x)) cnt--;
                    const int idx = cnt - 1 > 0 ? cnt - 1 : 0;
                    seg_lo = cnt > 0 ? sl.x(cnt - 1) : -__builtin_inf();
                    seg_hi = cnt < nk ? sl.x(cnt) : __builtin_inf();
                    sx = sl.x(idx); sa_ = cnt == 0 ? 0.0 : sl.a(idx); sb = sl.b(idx); sc_ = sl.c(idx); sy = sl.y(idx);
                }
                PP_DIAGC(1, true);
            }
            PP_REGION("eval");
            const double h = x - sx;
            // the left extrapolation (cnt == 0: x <= x0) is the cubic form with a = 0 (0 h + b = b, and
            // at x == x0, h = 0 both give y0); the right one (cnt == nk) uses the last knot, whose a is
            // 0 (spline.h:367): one polynomial form for every step
            const double y = ((sa_ * h + sb) * h + sc_) * h + sy;
            double d, rd;
            const bool dok = ppm::sqrt_rd((x - pos_x) * (x - pos_x) + (y - pos_y) * (y - pos_y), d, rd);
            double acc = fabs(speed - prev_speed) * 50;
            // the turn from the previous step direction u_prev to u = (dx, dy) / d (ppm::asin_small;
            // wide turns: atan2(u_prev x u, u_prev . u)). d == 0: atan2(+0, +0) = 0, u = (1, 0).
            double ux, uy;
            {
                PP_REGION("dir");
                const double ddx = x - pos_x, ddy = y - pos_y;
                ux = ddx * rd; uy = ddy * rd;
                PP_DIAGC(18, !dok);
                if (__builtin_expect(!dok, 0)) {        // d == 0 implies !dok (q = 0 < 2^-900)
                    PP_REGION("dirfix");
                    if (d == 0) { ux = 1.0; uy = 0.0; }
                    // finite step whose squared length overflows (speeds of ~1e150 m/s and more, only
                    // in k_cand<true> scenes): rd = 0 would leave no direction, where the reference's
                    // atan2(dy, dx) still has one; normalise the step scaled by its larger component
                    if (d == __builtin_inf() && fabs(ddx) <= 0x1.fffffffffffffp1023 &&
                        fabs(ddy) <= 0x1.fffffffffffffp1023) {
                        const double m = s_max(fabs(ddx), fabs(ddy));
                        const double a = ddx / m, b = ddy / m;
                        const double n = sqrt(a * a + b * b);
                        ux = a / n; uy = b / n;
                    }
                }
            }
            PP_REGION("cross");
            const double cr = uxp * uy - uyp * ux, dt = uxp * ux + uyp * uy;
            // the reference's wrap fmod(a + 3 pi, 2 pi) - pi: for |a| <= kStepSinMax, a + 3 pi lies in
            // [2 pi, 4 pi), where fmod is the exact subtraction of 2 pi (ppm::fmod_2pi's second case)
            double adiff;
            PP_DIAGC(3, !((PP_NARROW(dt, cr)) || speed == 0));
            PP_DIAGC(8, ng == 0 && !(PP_NARROW(dt, cr)));
            PP_DIAGC(9, !(dt > 0));
            if (__builtin_expect(PP_NARROW(dt, cr), 1)) {
                PP_REGION("asin");
                adiff = ((ppm::asin_small(cr) + 3 * kPi) - 2 * kPi) - kPi;
            } else {
                PP_REGION("wide");
                // cr, dt: components of unit vectors (finite, never both zero; NaN propagates)
                adiff = ppm::fmod_2pi_small(ppm::atan2_unit(cr, dt) + 3 * kPi) - kPi;
            }
            PP_REGION("acc");
            const double cacc = speed * 50 * fabs(adiff);
            double eff_c = cacc;
    #ifdef PP_LIMCENSUS
            bool cen_r1, cen_r2;
            {
                const double spd_r = sc_get_speed(sc, cur_t);                 // :919 (IEEE division)
                const double ast_r = ppg::atan2(y - pos_y, x - pos_x);        // :933
                const double adf_r = ppm::fmod_2pi(ast_r - ref_pa + 3 * kPi) - kPi;   // :934
                const double acc_r = fabs(spd_r - prev_speed) * 50, cacc_r = spd_r * 50 * fabs(adf_r);
                const double mx = P.maximum_acc, tol = 1e-12 * fabs(mx);
                cen_r1 = acc_r + cacc_r > mx;                                 // :941
                cen_r2 = cen_r1;
                if (cen_r1 && spd_r > prev_speed) {                           // :945-971, then :972
                    double na_r = mx - cacc_r;
                    if (na_r < 0) na_r = 0;
                    cen_r2 = na_r + cacc_r > mx;
                }
                PP_CEN(26, fabs(acc + cacc - mx) <= tol);
                PP_CEN(27, fabs(acc_r + cacc_r - mx) <= tol);
                PP_CEN(28, (acc + cacc > mx) != cen_r1);
                PP_CEN(32, __double_as_longlong(cacc) != __double_as_longlong(cacc_r));
                PP_CEN(33, __double_as_longlong(speed) != __double_as_longlong(spd_r));
                ref_pa = ast_r;
            }
    #endif
            PP_DIAGC(4, acc + cacc > P.maximum_acc);
            PP_DIAGC(10 + (ng == 0 ? 0 : ng == 1 ? 1 : ng < 5 ? 2 : ng < 10 ? 3 : ng < 20 ? 4 : 5), acc + cacc > P.maximum_acc);
            PP_DIAGC(5, acc + cacc > P.maximum_acc && speed > prev_speed);
            PP_DIAGC(7, acc + cacc > P.maximum_acc && speed > prev_speed && dcls == 1);
            if (acc + cacc > P.maximum_acc) {
                PP_REGION("lim");
                if (speed > prev_speed) {                                   // :945-971
                    PP_REGION("ovr");
                    // (inside this block acc + cacc > max held: neither is NaN; k_cand<false>'s
                    // operands are finite, so the clamp is v_max_f64)
                    double na = P.maximum_acc - cacc;
                    if (kLarge) { if (na < 0) na = 0; } else na = __builtin_fmax(na, 0.0);
                    const double ns = prev_speed + PP_DIV50(na);
                    sc_override_r<kLarge>(sc, cur_t, ns, rds);
                    speed = ns;
                    sc.ttime += 0.02;
                    rtt = ppm::rcp_nr(sc.ttime);
                    dstep = PP_DIV50(speed);
                    acc = na;
                    R.flags |= PP_ST_ACC_OVERRIDE;
                }
                PP_DIAGC(6, acc + cacc > P.maximum_acc);
                PP_CEN(29, true);
                PP_CEN(30, fabs(acc + cacc - P.maximum_acc) <= 1e-12 * fabs(P.maximum_acc));
                PP_CEN(31, cen_r1 && (acc + cacc > P.maximum_acc) != cen_r2);
                PP_REGION("lim2");
                if (acc + cacc > P.maximum_acc) {                           // :972-1018
                    PP_REGION("adj");
                    double nc = P.maximum_acc - acc;
                    if (kLarge) { if (nc < 0) nc = 0; } else nc = __builtin_fmax(nc, 0.0);
                    if (kOutMode == 2) {
                        // the output frame turns about the current point (src/main.cpp:986-997)
                        double cr, sr;
                        turn_sincos<kLarge>(turn_angle<kLarge>(nc, speed, adiff), sr, cr);
                        frame_turn(F, pos_x, pos_y, cr, sr);
                    } else if (kOutMode == 4) {
                        PP_DIAGC(19, !(!kLarge && PP_NARROW(dt, cr)));
                        PP_DIAGC(23, !kLarge && PP_NARROW(dt, cr));
                        if (!kLarge && PP_NARROW(dt, cr)) {
                            PP_REGION("adjn");
                            turn_narrow(F.ca, F.sa, nc, speed, adiff, dt, cr);
                        } else {
                            PP_REGION("adjwide");
                            double crr, srr;
                            turn_sincos<kLarge>(kLarge ? turn_angle<true>(nc, speed, adiff)
                                                       : turn_angle_fast(nc, speed, adiff), srr, crr);
                            frame_rot(F.ca, F.sa, crr, srr);
                        }
                    }
                    if (kOutMode == 3 && kRec) {
                        // the turn angle for k_emit's replay of the output frame
                        double* rp = rec_rot(rec - rs, rstride, ng, ws, rs);
                        if (PP_CHKP(rp, rec, nrec, 6))
                            PP_ST(rp, turn_angle<kLarge>(nc, speed, adiff));   // rot (src/main.cpp:986)
                        const uint64_t bit = 1ull << (ng & 63);
                        if (ng < 64) R.adj0 |= bit; else R.adj1 |= bit;
                    }
                    eff_c = nc;
                    R.flags |= PP_ST_CURV_ADJUST;
                }
            }
            PP_REGION("tail");
            cur_t += 0.02;
            psn = speed;
            uxn = ux; uyn = uy;
            double sp_step, dpy;
            if (kLarge) {
                sp_step = ppm::div_rcp_n((x - pos_x) * dstep, d, rd, dok);
                dpy = ppm::div_rcp_n((y - pos_y) * dstep, d, rd, dok);
            } else {          // ppm::div_rcp_d for both numerators, one !dok branch
                const double nx = (x - pos_x) * dstep, ny = (y - pos_y) * dstep;
                const double qx = nx * rd, qy = ny * rd;
                sp_step = __builtin_fma(__builtin_fma(-qx, d, nx), rd, qx);
                dpy = __builtin_fma(__builtin_fma(-qy, d, ny), rd, qy);
                if (__builtin_expect(!dok, 0)) { PP_REGION("tailfix"); sp_step = nx / d; dpy = ny / d; }
            }
            PP_REGION("tail2");
            pos_y += dpy;
            arg += sp_step;
            pos_x = arg;      // == pos_x + sp_step: both start at 0 and add the same sp_step (:1027-1031)
            if (kOutMode != 0 && kOut) {
                PP_REGION("out");
                PP_DIAGC(22, wx != nullptr);
                double ox, oy;
                if (kOutMode == 4) { ox = opx; oy = opy; frame_step(F.ca, F.sa, sp_step, dpy, ox, oy); }
                else frame_pt(F, pos_x, pos_y, ox, oy);
                if (wx && PP_CHKP(wx + ng * ws, nx, nnext, 1) && PP_CHKP(wy + ng * ws, ny, nnext, 2)) { PP_REGION("outw"); wx[ng * ws] = ox; wy[ng * ws] = oy; }
                PP_REGION("out2");
                if (px && PP_CHKP(px + ng * ps, paths, npaths, 3) && PP_CHKP(px + ng * ps + 1, paths, npaths, 3))
                    st_xy(px + ng * ps, ox, oy);      // one 16-B store (x, y)
                if (kOutMode == 4) { opx = ox; opy = oy; }
            }
            if (kOutMode == 3 && kRec && PP_CHKP(rec_px(rec - rs, rstride, ng, ws, rs), rec, nrec, 4) && PP_CHKP(rec_py(rec - rs, rstride, ng, ws, rs), rec, nrec, 5)) rec_st(rec - rs, rstride, ng, ws, rs, pos_x, pos_y);
            PP_REGION("latch");
            ng++;
            R.acc_sum += acc + eff_c;
            R.travelled += dstep;
        };
    double uxq = 0, uyq = 0, psq = 0;
    while (arg < 50 && ng < room) {
        step(uxp, uyp, prev_speed, uxq, uyq, psq);
        if (!(arg < 50 && ng < room)) break;
        step(uxq, uyq, psq, uxp, uyp, prev_speed);
    }
    PP_REGION("end");
    R.ng = ng;
    return R;
}

// per-candidate cost (identical formula in oracle/pp_oracle.c cand_cost)
__device__ __forceinline__ double cand_cost(const pp_params& P, const CandRes& R, int K, double score_L,
                                            int L, int T, double v, int open_mask, int ego_lane,
                                            uint32_t& flags) {
    const double acc_mean = R.ng > 0 ? R.acc_sum / R.ng : 0.0;
    const double ideal = (P.n_points - K) * P.max_speed / 50;
    const double deficit = 1.0 - R.travelled / ideal;
    double J = (2.5 - score_L) + acc_mean / P.maximum_acc + deficit + ((R.flags & PP_ST_FALLBACK) ? 1.0 : 0.0);
    if (!(J == J) || (R.flags & PP_ST_NAN)) { J = 999.0; flags |= PP_ST_NAN; }
    if (J > 999.0) J = 999.0;
    if (J < 0.0) J = 0.0;
    if (P.cost_mode == PP_COST_REFERENCE) {
        if (L != T) J += 1e6;
        if (v != P.max_speed) J += 1e3;
    } else {
        if (!((open_mask >> L) & 1) && L != ego_lane) J += 10.0;
    }
    return J;
}

__device__ __forceinline__ SC make_sc(const pp_params& P, const PrepV& pv, int64_t S, int64_t s,
                                      int L, double v) {
    SC sc;                                        // SpeedController ctor (src/main.cpp:495-502)
    sc.shift = 0;
    sc.start = pv.ego_speed[s];
    sc.target = v;
    sc.ttime = fabs(sc.start - v) / P.relaxed_acc;
    const int lm = pv.lim_mask[s];
    if (lm & 1) sc_add_limit(sc, pv.in_ts[s], pv.in_tt[s]);            // :1425-1431
    if (lm & (2 << L)) sc_add_limit(sc, pv.l_ts[L * S + s], pv.l_tt[L * S + s]);  // :1432-1438
    return sc;
}


// K4 inside k_cand (reference mode, emit_in): the winner lane of scene s replays the output
// transform of its recorded path (src/main.cpp:994-1007, 1033-1037) with the sin/cos of each
// recorded turn already in LDS (pcr/psr, one entry per step, computed by the block's team as
// emit_scene computes them): only the chain of turns and points is left to the lane. Operations
// and order are emit_scene's, so the outputs are bit-identical to the k_emit path.
template <int kChunk>
__device__ __forceinline__ void emit_scene_pre(const pp_scene_batch& in, const pp_params& P,
                                               const PrepV& pv, const pp_result& out, const double* rec,
                                               int64_t s, int K, int ng, uint64_t m0, uint64_t m1,
                                               const double* pcr, const double* psr) {
    const int64_t S = in.n_scenes;
    const int N = P.n_points;
    const int64_t rstride = (int64_t)(N - K) * S;
    {   // the kept previous points: every load issued before the first store
        double kx[PP_PREV_KEEP], ky[PP_PREV_KEEP];
#pragma unroll
        for (int i = 0; i < PP_PREV_KEEP; i++)
            if (i < K) { kx[i] = in.prev_x[(int64_t)i * S + s]; ky[i] = in.prev_y[(int64_t)i * S + s]; }
#pragma unroll
        for (int i = 0; i < PP_PREV_KEEP; i++)
            if (i < K) { PP_ST(out.next_x + (int64_t)i * S + s, kx[i]); PP_ST(out.next_y + (int64_t)i * S + s, ky[i]); }
    }
    OutFrame F = {pv.pos_x[s], pv.pos_y[s], pv.ca_p[s], pv.sa_p[s]};
    double pxp = 0, pyp = 0;                       // local position before the step
    for (int g0 = 0; g0 < ng; g0 += kChunk) {
        double px_[kChunk], py_[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; u++) {
            const int g = g0 + u;
#ifdef PP_CHECK
            if (g < ng) { PP_CHKP(rec_py((double*)rec, rstride, g, S, s), rec, nrec, 19); }
#endif
            px_[u] = 0.0; py_[u] = 0.0;
            if (g < ng) rec_ld(rec, rstride, g, S, s, px_[u], py_[u]);
        }
#pragma unroll
        for (int u = 0; u < kChunk; u++) {
            const int g = g0 + u;
            if (g >= ng) break;
            if ((g < 64 ? (m0 >> g) & 1 : (m1 >> (g - 64)) & 1) != 0) frame_turn(F, pxp, pyp, pcr[g], psr[g]);
            double ox, oy;
            frame_pt(F, px_[u], py_[u], ox, oy);
            if (!PP_CHKP(out.next_x + (int64_t)(K + g) * S + s, nx, nnext, 17)) break;
            PP_ST(out.next_x + (int64_t)(K + g) * S + s, ox);
            PP_ST(out.next_y + (int64_t)(K + g) * S + s, oy);
            pxp = px_[u];
            pyp = py_[u];
        }
    }
    for (int i = K + ng; i < N; i++) { out.next_x[(int64_t)i * S + s] = 0; out.next_y[(int64_t)i * S + s] = 0; }
}

// ------------------------------------------------------------------------------------------------
// K2: candidates. One workgroup = SPB scenes x C candidates; slots in LDS.
// kSlow = false: every scene except those flagged kLimSlow by k_prep (no library call in the
// loop, so the register peak stays at the loop's own state); kSlow = true: only flagged scenes.
// kMode 2: every candidate writes its path (emit_paths); 1: reference mode, the winner lanes
// write next_x/next_y; 0: cost only (comfort mode; k_winner produces the outputs).
// ------------------------------------------------------------------------------------------------
// k_winner's blocks and spline slots (kWinKnots = 9 previous + 6 control points, the real maximum)
constexpr int kWinBlock = 64;
constexpr int kWinKnots = 15;
static_assert(PP_PREV_KEEP - 1 + 6 <= kWinKnots && kWinKnots <= kKP, "slot too small");
constexpr int kWinRec = 5 * kWinKnots + 3;    // stored winner slot per scene (doubles): knots, 4 meta ints, pad (16-B records)
// ---- pieces of cand_group (those that could become functions of their own without a change to
// any kernel's machine code; the rest of it stays one body, in the order of its comments) ----

// The block's LDS as cand_group carves it (the layout is CandLds's, pp_k_spline.h): the slots, their
// meta ints, per scene the status flags and the slow marks, each winner's adjusted-step masks and
// step count for the in-block K4 (comfort mode keeps the scenes' winning candidates in sNg), and
// comfort mode's cost per lane
struct CandSm {
    double* sX;
    int* sMeta;
    uint32_t *sFlags, *sSlow;
    uint64_t* sAdj;
    int* sNg;
    double* sCost;
};

// a winner that writes next_x/next_y itself: the kept previous points, then where its loop writes
__device__ __forceinline__ void win_head(const pp_scene_batch& in, const pp_result& out, int64_t S, int64_t s,
                                         int K, double*& wx, double*& wy) {
    for (int i = 0; i < K; i++) {
        if (!PP_CHKP(out.next_x + (int64_t)i * S + s, nx, nnext, 9)) break;
        out.next_x[(int64_t)i * S + s] = in.prev_x[(int64_t)i * S + s];
        out.next_y[(int64_t)i * S + s] = in.prev_y[(int64_t)i * S + s];
    }
    wx = out.next_x + (int64_t)K * S + s;
    wy = out.next_y + (int64_t)K * S + s;
}
// ... and after its loop: the tail zeroed, its length and candidate
__device__ __forceinline__ void win_tail(const pp_result& out, int64_t S, int64_t s, int N, int K, int ng, int c) {
    for (int i = K + ng; i < N; i++) {
        if (!PP_CHKP(out.next_x + (int64_t)i * S + s, nx, nnext, 10)) break;
        out.next_x[(int64_t)i * S + s] = 0; out.next_y[(int64_t)i * S + s] = 0;
    }
    out.n_out[s] = K + ng;
    out.winner[s] = c;
}

// the scenes' status words: k_prep's flags and what the scene's candidates added
template <bool kSlow>
__device__ __forceinline__ void cand_status(const PrepV& pv, const pp_result& out, const CandSm& L, int64_t s0,
                                            int nsc, int D, int BPS, int tid) {
    if (tid < nsc && ((L.sSlow[tid] != 0) == kSlow) && PP_CHK(s0 + tid < g_lim.nscen, 15, s0 + tid)) {
        const uint32_t st = (uint32_t)pv.status[(s0 + tid) * D] | L.sFlags[tid];
        if (BPS == 1) out.status[s0 + tid] = st;
        else atomicOr(&out.status[s0 + tid], st);     // zeroed by k_prep
    }
}

// comfort mode, after the block's decision: the winner's spline slot copied from LDS to the
// stored-slot buffer, so k_winner_st re-runs the winner without building its spline a second time (the slot is what setup_lane
// builds, element for element). The scene's record: the LDS slot's knot-interleaved doubles (x, y,
// a, b, c of knot i at 5 i + field) as they lie, then the 4 meta ints; consecutive threads copy
// consecutive items of a scene, so a wave stores contiguous bytes
template <bool kSlow>
__device__ __forceinline__ void cand_store_slot(const CandSm& L, int nslot, double* wslot, int64_t s0, int nsc,
                                                int NS, int tid) {
    constexpr int kItems = 5 * kWinKnots + 4;
    for (int idx = tid; idx < nsc * kItems; idx += (int)blockDim.x) {
        const int w = idx / kItems, e = idx - w * kItems;
        if ((L.sSlow[w] != 0) != kSlow) continue;
        const int64_t s = s0 + w;
        const Slot sl = lds_slot(L.sX, nslot, L.sMeta, w * NL + L.sNg[w] / NS);
        double* rec_s = wslot + s * kWinRec;
        if (e < 5 * kWinKnots) rec_s[e] = sl.X[e];
        else ((int*)(rec_s + 5 * kWinKnots))[e - 5 * kWinKnots] = sl.m(e - 5 * kWinKnots);
    }
}

// One group g of the candidate grid (BPS == 1: scenes [g SPB, g SPB + SPB); BPS > 1: candidates
// [coff, coff + 256) of scene g / BPS) by the whole workgroup. Every barrier inside is reached by
// all threads of the block (the early return is block-uniform).
// kEmitIn (reference mode, kMode 1): 0 the winners' paths are replayed by k_emit; 1 by the block
// after phase B (K4 in the block, below); 2 the winner lanes write their points during the loop
// (output mode 2: the transform and its turns in the step, no record and no replay — the
// single-frame and small-batch step, whose time is the winners' serial chain)
// kPreA: the block's (single) scene has its fast-path spline slots built already (k_plan_frame's
// second wave builds them while the first runs K1): phase A is skipped
// kLoop: the caller runs group after group in one block (the persistent k_cand): the thread index
// is taken through an empty asm statement, so the compiler computes the per-thread set-up where
// each group uses it, as in the one-group kernels, and does not carry it in registers across the
// candidate loop (hoisted out of the caller's loop it spills there)
// kShape: the group's shape is BASELINE config 5's, as compile-time constants (kShapeNS speeds, no
// draws, kShapeSPB scenes per group in 256 threads, teams of kShapeTS): only the integer index
// arithmetic, the loop bounds and the LDS pointer arithmetic change; the caller passes SPB =
// kShapeSPB and BPS = 1 and has checked P.n_speeds and the block size
constexpr int kShapeNS = 5, kShapeSPB = 17, kShapeTS = 256 / (NL * kShapeSPB) > 8 ? 8 : 256 / (NL * kShapeSPB);
template <bool kSlow, int kMode, int kEmitIn = 0, bool kPreA = false, bool kLoop = false, bool kShape = false>
__device__ __forceinline__ void cand_group(const MapG& mg, const pp_scene_batch& in, const pp_params& P,
                                           const PrepV& pv, const pp_result& out, int SPB, int BPS,
                                           double* rec, uint64_t* adjm, int64_t g, double* sm,
                                           double* wslot = nullptr) {
    constexpr bool emit_in = kEmitIn == 1 && kMode == 1;
    constexpr bool win_inline = kEmitIn == 2 && kMode == 1;
    const int NS = kShape ? kShapeNS : P.n_speeds, Cv = NL * NS, N = P.n_points;
    const int D = kShape ? 1 : P.n_draws > 1 ? P.n_draws : 1;
    const int C = D * Cv;                     // candidates per scene (all draws)
    const int nslot = NL * SPB;
    // the block's LDS: CandLds's layout (pp_k_spline.h: the host's sizes and the step kernels' geometry
    // records come from there). The pointers are still derived here, in the form that leaves every
    // kernel's machine code as it was; a change to either place needs the same change in the other
    double* sX = sm;
    double* sY = sX + nslot * kKP;
    double* sA = sY + nslot * kKP;
    double* sB = sA + nslot * kKP;
    double* sC = sB + nslot * kKP;
    int* sMeta = (int*)(sC + nslot * kKP);
    uint32_t* sFlags = (uint32_t*)(sMeta + 4 * nslot);
    const MapV m = map_view(mg.buf, mg.n);
    const int64_t S = in.n_scenes;
    const int64_t Sv = S * D;
    // block -> scenes: BPS == 1: SPB whole scenes; BPS > 1 (C > 256): one scene, candidates
    // [coff, coff + 256) of it; BPS < 0 (kMode 2, the flat geometry): the batch's candidates
    // [256 g, 256 g + 256), from candidate coff of scene s0 on, over at most SPB scenes
    int64_t s0;
    int coff;
    int nsc;
    if (BPS == 1) { s0 = g * SPB; coff = 0; }
    else if (BPS < 0) { s0 = g * 256 / C; coff = (int)(g * 256 - s0 * C); }
    else { s0 = g / BPS; coff = (int)(g - s0 * BPS) * 256; }
    if (BPS < 0) {
        const int span = (coff + 255) / C + 1;
        nsc = (int)((S - s0) < span ? (S - s0) : span);
    } else {
        nsc = (int)((S - s0) < SPB ? (S - s0) : SPB);
    }
    int tid = threadIdx.x;
    if (kLoop) asm volatile("" : "+v"(tid));
    // per scene: any of its draws flagged kLimSlow (absurd heading, or a speed or ramp time outside
    // the range of the unchecked divisions) -> the scene runs in the k_cand<true> instantiation
    uint32_t* sSlow = sFlags + SPB;
    // kMode 1 with emit_in: each winner's step count and adjusted-step masks for the in-block K4
    uint64_t* sAdj = (uint64_t*)(((uintptr_t)(sSlow + SPB) + 7) & ~(uintptr_t)7);
    int* sNg = (int*)(sAdj + 2 * SPB);
    // comfort mode with a stored winner slot: each lane's cost (the host sizes the LDS for it)
    double* sCost = (double*)(((uintptr_t)(sNg + SPB) + 7) & ~(uintptr_t)7);
    if (tid < SPB) { sFlags[tid] = 0; sSlow[tid] = 0; }
#ifdef PP_TRACE
    if (!kSlow && tid == 0) {
        PP_TRACE_AT(blockIdx.x, 0);
        if (blockIdx.x < (unsigned)kTraceK1) g_trace[8 * blockIdx.x + 7] = trace_hwid();
    }
#endif
#ifdef PP_CHECK
    if (!kPreA) {
        for (int i = tid; i < 5 * nslot * kKP; i += (int)blockDim.x) sX[i] = __builtin_nan("");
        for (int i = tid; i < 4 * nslot; i += (int)blockDim.x) sMeta[i] = kMetaPoison;
    }
#endif
    __syncthreads();
    bool mine = false;
    for (int t = tid; t < nsc * D; t += (int)blockDim.x) {
        const int q = t / D;
        if (pv.lim_mask[(s0 + q) * D + (t - q * D)] & kLimSlow) { atomicOr(&sSlow[q], 1u); mine = true; }
    }
    // (kLoop is k_cand<false>'s: the vote's result is not used there, only its barrier; the vote's
    // flat thread index would otherwise stay in registers from group to group)
    if (kLoop && !kSlow) __syncthreads();
    else if (!__syncthreads_or(mine) && kSlow) return;      // whole block leaves: no flagged scene
    if (!kPreA) {   // phase A: a team of TS threads per slot (team_a1..a5), block barriers between the steps
        int TS = kShape ? kShapeTS : (int)blockDim.x / nslot;
        if (TS > 8) TS = 8;
        const int j = tid / TS, r = tid - j * TS;
        const bool act = j < NL * nsc && ((sSlow[j / NL] != 0) == kSlow);
        const Slot sl = lds_slot(sX, nslot, sMeta, j);
        const int L = j % NL;
        const int64_t s = s0 + j / NL;
        LaneGeom g;
        PP_REGION_A("a1");
        if (act) { g = lane_geom(pv, s * D, Sv, L); team_a1(m, in, g, s, L, sl, r, TS); }
        __syncthreads();
        PP_REGION_A("a2");
        // the two serial steps (A2, A4) on one lane per slot, slots in lane order: NL * SPB <= 64
        // slots fit the block's first wave, whose instruction stream is then the only one paying
        // for them (a team layout spreads them over every wave of the block)
        const int js = tid;
        const bool act_s = js < NL * nsc && ((sSlow[js / NL] != 0) == kSlow);
        const Slot sls = lds_slot(sX, nslot, sMeta, js);
        if (act_s) {
            const int64_t vs = (s0 + js / NL) * D;
            LaneGeom gs;
            gs.K = pv.K[vs];
            gs.npk = gs.K > 0 ? gs.K - 1 : 0;
            gs.pos_x = pv.pos_x[vs]; gs.pos_y = pv.pos_y[vs]; gs.ego_d = pv.ego_d[vs];
            team_a2(gs, sls);
        }
        __syncthreads();
        PP_REGION_A("a3");
        if (act) team_a3(sl, r, TS);
        __syncthreads();
        PP_REGION_A("a4");
        if (act_s) team_a4(sls);
        __syncthreads();
        PP_REGION_A("a5");
        if (act) team_a5(sl, r, TS);
    }
    PP_REGION_A("pre");
    __syncthreads();
    if (!kSlow && tid == 0) PP_TRACE_AT(blockIdx.x, 1);
    // Lane -> candidate. Reference mode without draws (kMode 1): lanes [0, nsc) run the scenes'
    // winning candidates (planner lane T, max_speed: known from k_prep) and record their paths;
    // lanes >= nsc run the C - 1 other candidates of each scene cost-only. The output work is
    // thereby confined to the block's first wave; the other waves run the lean cost-only loop.
    int sc_l, c;
    if (kMode == 1) {
        if (tid < nsc) {
            sc_l = tid;
            c = pv.T[s0 + tid] * NS;
        } else {
            const int t2 = tid - nsc;
            sc_l = t2 / (C - 1);
            const int r = t2 - sc_l * (C - 1);
            const int cw = sc_l < nsc ? pv.T[s0 + sc_l] * NS : 0;
            c = r < cw ? r : r + 1;
        }
    } else {
        const int t = tid + coff;
        sc_l = t / C;
        c = t - sc_l * C;
    }
    if (sc_l < nsc && c < C && ((sSlow[sc_l] != 0) == kSlow)) {   // phase B
        const int64_t s = s0 + sc_l;
        const int d = c / Cv, cc = c - d * Cv;
        const int64_t v = s * D + d;              // this draw's prep record
        const int L = cc / NS, k = cc - L * NS;
        const int j = sc_l * NL + L;
        const Slot sl = lds_slot(sX, nslot, sMeta, j);
#ifdef PP_CHECK
        {   // the slot was written by this group's phase A (not left over from an earlier group)
            const int nk_ = sl.m(0), ncp_ = sl.m(1), npk_ = sl.m(2);
            chk_(j < nslot && nk_ != kMetaPoison && nk_ >= 1 && nk_ <= kKP && ncp_ >= 1 && ncp_ <= 6 &&
                 npk_ >= 0 && npk_ < PP_PREV_KEEP, 20, j, g);
        }
#endif
        const double vt = cand_speed(P, pv.ego_speed[v], k);
        const SC sc = make_sc(P, pv, Sv, v, L, vt);
        const int K = pv.K[v], T = pv.T[v];
        // reference mode: the winning candidate (planner lane, max_speed) is known before the
        // loop, so its lane writes next_x/next_y (point-major) during the same pass
        const bool winner = kMode == 1 ? tid < nsc
                                       : (kMode == 2 && P.cost_mode == PP_COST_REFERENCE && L == T && k == 0);
        CandRes R;
        if (kMode == 2) {
            // every candidate writes its path; in reference mode the winner also writes next_x/y
            double* wx = nullptr;
            double* wy = nullptr;
            if (winner) win_head(in, out, S, s, K, wx, wy);
            const int64_t ps = (int64_t)C * 2;
            double* p0 = out.paths + ((s * N) * C + c) * 2;
            for (int i = 0; i < K; i++) {
                if (!PP_CHKP(p0 + i * ps + 1, paths, npaths, 7)) break;
                st_xy(p0 + i * ps, in.prev_x[(int64_t)i * S + s], in.prev_y[(int64_t)i * S + s]);
            }
            double* px = p0 + K * ps;
#ifdef PP_DIAG_NOB
            // diagnostic builds only: phase B skipped (wrong results; measures everything else)
            R = CandRes{0, 0, N - K, 0, 0, 0};
            (void)sc; (void)wx; (void)wy;
#else
            R = run_candidate<kSlow, 4>(P, sl, pv.pos_x[v], pv.pos_y[v], pv.angle[v],
                                                       pv.ca_p[v], pv.sa_p[v], sc, N - K, wx, wy, S,
                                                       px, ps);
#endif
            for (int i = R.ng; i < N - K; i++) {
                if (!PP_CHKP(px + i * ps + 1, paths, npaths, 8)) break;
                st_xy(px + i * ps, __builtin_nan(""), __builtin_nan(""));
            }
            if (out.path_len && PP_CHK(s * C + c < g_lim.ncost, 11, s * C + c)) out.path_len[s * C + c] = K + R.ng;
            if (winner) win_tail(out, S, s, N, K, R.ng, c);
        } else if (win_inline && tid < 64) {
            // reference mode, the block's first wave: the winners write next_x/next_y in the loop
            // (the rest of the wave runs the same instantiation without outputs, in lockstep)
            double* wx = nullptr;
            double* wy = nullptr;
            if (winner) win_head(in, out, S, s, K, wx, wy);
            R = run_candidate<kSlow, 2>(P, sl, pv.pos_x[v], pv.pos_y[v], pv.angle[v], pv.ca_p[v], pv.sa_p[v],
                                        sc, N - K, wx, wy, S, nullptr, 0);
            if (winner) win_tail(out, S, s, N, K, R.ng, c);
        } else if (kMode == 1 && tid < 64) {
            // reference mode, the block's first wave: the winners record their local path
            // (3 stores per step) for k_emit; the other lanes of the wave are cost-only
#ifdef PP_DIAG_NOB
            R = CandRes{0, 0, N - K, 0, 0, 0};   // (diagnostic builds: phase B skipped)
#else
            R = run_candidate<kSlow, 3>(P, sl, 0, 0, 0, 1, 0, sc, N - K, nullptr, nullptr,
                                                       S, nullptr, 0, winner, rec + s, 0, s);
#endif
            if (winner && emit_in) {          // in-block K4 below: step count and masks in LDS
                out.n_out[s] = K + R.ng;
                out.winner[s] = c;
                sNg[sc_l] = R.ng; sAdj[2 * sc_l] = R.adj0; sAdj[2 * sc_l + 1] = R.adj1;
            } else if (winner && PP_CHK(s < g_lim.nscen, 12, s) && PP_CHKP(adjm + S + s, adjm, nadj, 13)) {
                out.n_out[s] = K + R.ng;
                out.winner[s] = c;
                adjm[s] = R.adj0;
                adjm[S + s] = R.adj1;
            }
        } else {
#ifdef PP_DIAG_NOB
            R = CandRes{0, 0, N - K, 0, 0, 0};   // (diagnostic builds: phase B skipped)
#else
            R = run_candidate<kSlow, 0>(P, sl, 0, 0, 0, 1, 0, sc, N - K,
                                                       nullptr, nullptr, 0, nullptr, 0, true, nullptr,
                                                       fabs(sc.target - sc.start) >= 7.5 * sc.ttime ? 2 : (sc.target > sc.start ? 1 : 0));
#endif
        }
        PP_REGION_A("post");
        uint32_t flags = R.flags;
        const double cost = cand_cost(P, R, K, pv.score[L * Sv + v], L, T, vt, pv.open_mask[v],
                                      pv.ego_lane[v], flags);
        if (PP_CHKP(out.cost + s * C + c, cost, ncost, 14)) out.cost[s * C + c] = cost;
        if (kMode == 0 && wslot && BPS == 1 && D == 1) sCost[tid] = cost;     // (k_winner_st's decision)
        if (D > 1) flags |= (uint32_t)pv.status[v];     // every draw's planner flags
        atomicOr(&sFlags[sc_l], flags);
    }
    if (!kSlow && (tid & 63) == 0 && tid < 256) PP_TRACE_AT(blockIdx.x, 2 + (tid >> 6));
    __syncthreads();
    const CandSm lds = {sX, sMeta, sFlags, sSlow, sAdj, sNg, sCost};
    cand_status<kSlow>(pv, out, lds, s0, nsc, D, BPS, tid);
    if (!kSlow && tid == 0) PP_TRACE_AT(blockIdx.x, 6);
    if (kMode == 0 && wslot && BPS == 1 && D == 1) {
        // comfort mode (every candidate of the block's scenes in this block, no draws): the
        // per-scene decision, k_winner's rule (first minimum over (lane, speed)) over the costs the
        // lanes left in LDS, then the winner's spline slot to the stored-slot buffer
        int* sBest = sNg;
        if (tid < nsc && ((sSlow[tid] != 0) == kSlow)) {
            int best = 0;
            double bc = 0;
            for (int cc = 0; cc < Cv; cc++) {
                const double cst = sCost[tid * C + cc];
                if (cc == 0 || cst < bc) { bc = cst; best = cc; }
            }
            sBest[tid] = best;
            out.winner[s0 + tid] = best;
        }
        __syncthreads();
        cand_store_slot<kSlow>(lds, nslot, wslot, s0, nsc, NS, tid);
    }
    if (kMode == 1 && emit_in) {
        // K4 in the block (reference mode): the spline slots are free now, so the team computes
        // the sin/cos of every recorded turn of the block's winners into them (one item per
        // winner x step), then each winner lane replays its transform from its own record
        // (emit_scene_pre: the chain of turns and points only, emit_scene's operations).
        double* pcr = sm;
        double* psr = sm + SPB * N;               // (CandLds::replay_fits: the host asks it before this launch)
        for (int idx = tid; idx < nsc * N; idx += (int)blockDim.x) {
            const int w = idx / N, gs = idx - w * N;
            if (((sSlow[w] != 0) != kSlow) || gs >= sNg[w]) continue;
            const uint64_t mm = gs < 64 ? sAdj[2 * w] : sAdj[2 * w + 1];
            if (!((mm >> (gs & 63)) & 1)) continue;
            const int64_t s = s0 + w;
            const double* rr = rec_rot(rec, (int64_t)(N - pv.K[s]) * S, gs, S, s);
            if (!PP_CHKP(rr, rec, nrec, 18)) continue;
            const double rt = *rr;
            double sr, cr;
            turn_sincos<true>(rt, sr, cr);
            pcr[idx] = cr; psr[idx] = sr;
        }
        __syncthreads();
        if (!kSlow && tid == 0) PP_TRACE_AT(blockIdx.x, 7);
        if (tid < nsc && ((sSlow[tid] != 0) == kSlow)) {
            const int64_t s = s0 + tid;
            emit_scene_pre<kEmitChunk>(in, P, pv, out, rec, s, pv.K[s], sNg[tid], sAdj[2 * tid],
                                          sAdj[2 * tid + 1], pcr + tid * N, psr + tid * N);
        }
    }
}

// k_cand<false>: the full grid, one group per workgroup; scenes k_prep flagged kLimSlow are left
// to k_cand<true>, which runs only the groups whose bit k_prep set in `gbits` (a bitmap over the
// groups): gridDim.x workgroups walk the bitmap with stride gridDim.x (the bit test and the loop
// are block-uniform; a barrier separates consecutive groups' use of the block's LDS). Each group
// clears its bit after use, so the bitmap is all zero again for the next pp_eval.
template <bool kSlow, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kCandWaves))) void k_cand(MapG mg, pp_scene_batch in, pp_params P, PrepV pv,
                                              pp_result out, int SPB, int BPS, double* rec, uint64_t* adjm,
                                              uint32_t* gbits, int64_t ngroups, const uint32_t* glist,
                                              const uint32_t* gcount, int64_t g0, double* wslot) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if (!kSlow) {
        cand_group<false, kMode>(mg, in, P, pv, out, SPB, BPS, rec, adjm, g0 + blockIdx.x, sm, wslot);
        return;
    }
    // the flagged groups k_prep listed (each listed once: the first setter of its bit appends it)
    const uint32_t nl = *gcount;                                  // same address for every lane
    for (uint32_t i = blockIdx.x; i < nl; i += gridDim.x) {
        const int64_t g = glist[i];
        if (!PP_CHK(g < ngroups, 21, g)) continue;               // (never: k_prep lists this call's groups)
        __syncthreads();                                          // the previous group's LDS readers are done
        cand_group<true, kMode>(mg, in, P, pv, out, SPB, BPS, rec, adjm, g, sm, wslot);
        if (threadIdx.x == 0) atomicAnd(&gbits[g >> 5], ~(1u << (g & 31)));
    }
}

// The persistent fast path of reference mode (kMode 1 without paths or draws, large batches on one
// stream): the grid is the device's resident block count; block b runs group b, then the groups it
// claims from `next` (a counter of the stream's workspace that pp_eval zeroes ahead of K1: claim i
// is group gridDim.x + i), so a block's slot never waits for the dispatcher between two groups and
// the spread of the groups' times (53-81 us) is absorbed by the order of the claims. One thread
// claims; the group index reaches the block through the word behind the block's LDS
// (CandLds::bytes_persist), and the barrier of that broadcast is also the one that separates the
// previous group's LDS readers from the next group's writers. A block beyond the batch's groups
// leaves before it touches LDS. The groups themselves are cand_group<false, kMode>'s, bit for bit;
// flagged scenes are left to k_cand<true>, launched after this kernel as after k_cand<false>.
struct Persist {};
struct PersistShape {};       // the same with cand_group's kShape
// its arguments, one struct at offset 0 of the kernel-argument segment: each group reads what it
// needs from there through a pointer the compiler cannot follow across groups (scalar loads, as the
// one-group kernels issue them), because arguments held in scalar registers across the candidate
// loop overflow the scalar file into vector registers and those into scratch
struct PersistArgs {
    MapG mg; pp_scene_batch in; pp_params P; PrepV pv; pp_result out;
    int SPB; double* rec; uint64_t* adjm; int64_t ngroups; uint32_t* next;
};
template <class kTag, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kCandWaves))) void k_cand(PersistArgs a0) {
    static_assert(kMode == 1, "the persistent K2 is reference mode's");
    constexpr bool kShape = std::is_same<kTag, PersistShape>::value;
    typedef const __attribute__((address_space(4))) PersistArgs* KArg;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    int64_t g = blockIdx.x;
    if (g >= a0.ngroups) return;
    for (;;) {
        KArg ka = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const PersistArgs& a = *(const PersistArgs*)ka;
        cand_group<false, kMode, 0, false, true, kShape>(a.mg, a.in, a.P, a.pv, a.out, kShape ? kShapeSPB : a.SPB, 1, a.rec, a.adjm, g, sm, nullptr);
        uint32_t* sNext = (uint32_t*)(sm + CandLds{kShape ? kShapeSPB : a.SPB}.doubles());
        if (threadIdx.x == 0) *sNext = atomicAdd(a.next, 1u);
        __syncthreads();
        g = (int64_t)gridDim.x + *sNext;
        if (g >= a.ngroups) return;
    }
}
