// pp_k_spline.h — device: phase A, the control points and tk::spline coefficients of one (scene, lane)
// into a slot (TrajectoryBuilder::build's setup, src/main.cpp:575-904, spline.h:284-373): Slot,
// setup_lane (one lane per slot) and team_a1..a5 (a team of lanes per slot).
// Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// Phase A: control points + spline for one (scene, lane) into a slot
// ------------------------------------------------------------------------------------------------
// A slot holds one spline: knots X/Y and coefficients A/B/C (<= PP_MAX_KNOTS each) + 4 ints.
// k_cand keeps slots in LDS (stride 1); k_winner in a global scratch laid out [field][knot][S]
// (stride S: lanes of a wave touch consecutive addresses).
struct Slot {
    double *X, *Y, *A, *B, *C;
    int* meta;          // [0] n knots, [1] n control points, [2] first control-point knot, [3] flags
    int64_t st;         // element stride of the knot arrays
    int64_t mst;        // element stride of meta
    __device__ __forceinline__ double& x(int i) const { return X[i * st]; }
    __device__ __forceinline__ double& y(int i) const { return Y[i * st]; }
    __device__ __forceinline__ double& a(int i) const { return A[i * st]; }
    __device__ __forceinline__ double& b(int i) const { return B[i * st]; }
    __device__ __forceinline__ double& c(int i) const { return C[i * st]; }
    __device__ __forceinline__ int& m(int k) const { return meta[k * mst]; }
};
// k_cand's LDS slot j. PP_SLOT_AOS: knot-interleaved, knot i of slot j holds x, y, a, b, c at
// sm[(j * kKP + i) * 5 + field] — one address register per slot and immediate offsets for the five
// fields (the field-major layout needs five: in emit_paths mode they spill, and every reload waits
// for the lane's outstanding path stores). Otherwise field-major, sX[j * kKP + i] etc.
__device__ __forceinline__ Slot lds_slot(double* sX, int nslot, int* sMeta, int j) {
    (void)nslot;
    double* b = sX + (int64_t)j * kKP * 5;
    return Slot{b, b + 1, b + 2, b + 3, b + 4, sMeta + 4 * j, 5, 1};
}
// The LDS of a k_cand block of spb scenes: the host sizes every launch by it, decides by it whether
// the in-block replay fits, and the one-launch step puts its geometry records behind it
// (cand_group and wave_phase_a still derive their pointers themselves, in this order). In
// order (byte offsets from the block's first slot): the NL spb spline slots (5 kKP doubles each,
// knot-interleaved: lds_slot), their 4 meta ints each, then per scene the status flags and the
// slow marks, (8-aligned) each winner's two adjusted-step masks and its step count, and (8-aligned;
// comfort mode with a stored winner slot only) one cost per lane of the block.
constexpr int kCandCostLanes = 256;               // k_cand's largest block
struct CandLds {
    int spb;
    static __host__ __device__ constexpr size_t up8(size_t b) { return (b + 7) / 8 * 8; }
    __host__ __device__ constexpr int nslot() const { return NL * spb; }
    __host__ __device__ constexpr int slot_doubles() const { return 5 * kKP * nslot(); }   // the slot area
    __host__ __device__ constexpr size_t meta() const { return sizeof(double) * 5 * kKP * nslot(); }
    __host__ __device__ constexpr size_t flags() const { return meta() + sizeof(int) * 4 * nslot(); }
    __host__ __device__ constexpr size_t slow() const { return flags() + sizeof(uint32_t) * spb; }
    __host__ __device__ constexpr size_t adj() const { return up8(slow() + sizeof(uint32_t) * spb); }
    __host__ __device__ constexpr size_t ng() const { return adj() + sizeof(uint64_t) * 2 * spb; }
    __host__ __device__ constexpr size_t bytes() const { return ng() + sizeof(int) * spb; }
    __host__ __device__ constexpr size_t cost() const { return up8(bytes()); }
    __host__ __device__ constexpr size_t bytes_cost() const { return cost() + sizeof(double) * kCandCostLanes; }
    // whole doubles that cover bytes(): what follows the block's LDS starts there. (The kernels
    // evaluate this one; it is bytes() written out in the order that leaves their code as it was)
    __host__ __device__ constexpr int doubles() const {
        return (int)(((sizeof(double) * 5 * kKP * (NL * spb) + sizeof(int) * 4 * (NL * spb) + sizeof(uint32_t) * 2 * spb + 7) / 8 * 8 +
                      sizeof(uint64_t) * 2 * spb + sizeof(int) * spb + 7) / 8);
    }
    // K4 inside k_cand: once phase B is done the winners' sin/cos tables (N doubles each, two per
    // scene) overlay the slot area, so they have to fit it
    __host__ __device__ constexpr bool replay_fits(int N) const { return 2 * spb * N <= slot_doubles(); }
    // the persistent k_cand: one more word at doubles(), the group the block claimed
    __host__ __device__ constexpr size_t bytes_persist() const { return sizeof(double) * (size_t)doubles() + 8; }
};
// the persistent k_cand keeps four blocks on a CU (160 KB of LDS) at config 5's 17 scenes per block
static_assert(PP_NUM_LANES != 3 || 4 * CandLds{17}.bytes_persist() <= 160 * 1024, "four persistent k_cand blocks per CU");
#if PP_NUM_LANES == 3
static_assert(CandLds{1}.bytes() == 2116 && CandLds{4}.bytes() == 8464 && CandLds{16}.bytes() == 33856, "k_cand's LDS");
static_assert(CandLds{1}.bytes_cost() == 4168 && CandLds{4}.bytes_cost() == 10512 &&
              CandLds{16}.bytes_cost() == 35904, "k_cand's LDS with the cost array");
#elif PP_NUM_LANES == 4
static_assert(CandLds{1}.bytes() == 2812 && CandLds{4}.bytes() == 11248 && CandLds{16}.bytes() == 44992, "k_cand's LDS");
static_assert(CandLds{1}.bytes_cost() == 4864 && CandLds{4}.bytes_cost() == 13296 &&
              CandLds{16}.bytes_cost() == 47040, "k_cand's LDS with the cost array");
#endif
static_assert(8u * CandLds{1}.doubles() >= CandLds{1}.bytes() && 8u * CandLds{4}.doubles() >= CandLds{4}.bytes() &&
              8u * CandLds{16}.doubles() >= CandLds{16}.bytes(), "doubles() covers bytes()");
static_assert(CandLds{1}.doubles() == (CandLds{1}.bytes() + 7) / 8 && CandLds{4}.doubles() == (CandLds{4}.bytes() + 7) / 8 &&
              CandLds{16}.doubles() == (CandLds{16}.bytes() + 7) / 8, "doubles() is bytes() rounded up");
constexpr int kMetaFallback = 1, kMetaTrunc = 2, kMetaWalkFail = 4;

// s: scene (inputs, stride in.n_scenes); v: its prep record (stride Sv). The spline depends on the
// ego state only (no sensor-fusion input), so every Monte-Carlo draw of a scene shares it.
__device__ void setup_lane(const MapV& m, const pp_params& P, const pp_scene_batch& in,
                           const PrepV& pv, int64_t s, int64_t v, int64_t Sv, int L, const Slot& sl) {
    const int64_t S = in.n_scenes;
    const int K = pv.K[v];
    const double pos_x = pv.pos_x[v], pos_y = pv.pos_y[v];
    const double ca = pv.ca_m[v], sa = pv.sa_m[v];
    const double start = pv.ego_speed[v], ego_d = pv.ego_d[v], ego_vd = pv.ego_vd[v];
    const int ref_wp = pv.ref_wp[v];
    const double ratio = pv.ratio[L * Sv + v];
    int flags = 0;
    // lane switch time / first control point distance (src/main.cpp:640-731)
    double min_cpd = start * 1;
    min_cpd = s_max(min_cpd, 5.0);
    const double d_diff = lane_offset(L) - ego_d;
    const double d_acc = 4;
    bool slow = false;
    double lst = 2.0;
    if ((ego_vd < 0) == (d_diff < 0)) {
        const double dmax = ego_vd * ego_vd / d_acc / 2;
        if (dmax > fabs(d_diff)) { slow = true; lst = fabs(ego_vd) / d_acc; }
    }
    if (!slow) {
        double rel = ego_vd;
        if (d_diff < 0) rel *= -1;
        const double add = fabs(d_diff);
        const double peak = sqrt(add * d_acc + rel * rel / 2);
        lst = (peak * 2 - rel) / d_acc;
    }
    double dist = start * lst;
    if (dist < 10.0) dist = 10.0;
    if (dist > 50) dist = 50;
    // knots: previous points [0, K-1) then control points, all in the local frame (:786-831)
    const int npk = K > 0 ? K - 1 : 0;
    for (int i = 0; i < npk; i++) {
        const double tx0 = in.prev_x[(int64_t)i * S + s] - pos_x;
        const double ty0 = in.prev_y[(int64_t)i * S + s] - pos_y;
        sl.x(i) = tx0 * ca - ty0 * sa;
        sl.y(i) = tx0 * sa + ty0 * ca;
    }
    // control points (:638, 744-768): first = start pose, then get_lane_pos steps
    double lx = pos_x, ly = pos_y, total = 0;
    sl.x(npk) = (pos_x - pos_x) * ca - (pos_y - pos_y) * sa;
    sl.y(npk) = (pos_x - pos_x) * sa + (pos_y - pos_y) * ca;
    int ncp = 1;
    // the five candidate control points (:744-768); their lane positions in one walk when the
    // targets are positive (always, unless the telemetry speed is not finite)
    double cpsv[5], cpx[5], cpy[5];
    bool cok[5];
    cpsv[0] = dist;
    for (int i = 1; i < 5; i++) cpsv[i] = cpsv[i - 1] + min_cpd;
    if (cpsv[0] > 0 && cpsv[1] > 0 && cpsv[2] > 0 && cpsv[3] > 0 && cpsv[4] > 0) {
        get_lane_pos_multi<5>(m, ref_wp, ratio, cpsv, L, cpx, cpy, cok);
    } else {
        for (int i = 0; i < 5; i++) get_lane_pos(m, ref_wp, ratio, cpsv[i], L, cpx[i], cpy[i], cok[i]);
    }
    for (int i = 0; i < 5; i++) {
        const double npx = cpx[i], npy = cpy[i];
        if (!cok[i]) flags |= kMetaWalkFail;
        total += sqrt((npx - lx) * (npx - lx) + (npy - ly) * (npy - ly));
        lx = npx; ly = npy;
        const double tx0 = npx - pos_x, ty0 = npy - pos_y;
        sl.x(npk + ncp) = tx0 * ca - ty0 * sa;
        sl.y(npk + ncp) = tx0 * sa + ty0 * ca;
        ncp++;
        if (total > 50 && ncp > 2) break;
    }
    int nk = npk + ncp;
    for (int i = 1; i < nk; i++) {                                      // :833-843
        if (sl.x(i) <= sl.x(i - 1)) { nk = i; flags |= kMetaTrunc; break; }
    }
    const bool fallback = nk < 3 || nk <= npk || fabs(ego_d) > 20;      // :848
    if (fallback) flags |= kMetaFallback;
    sl.m(0) = nk; sl.m(1) = ncp; sl.m(2) = npk; sl.m(3) = flags;
    if (fallback) return;
    // tk::spline::set_points (spline.h:284-373): tridiagonal band LU, rows preconditioned,
    // no pivoting. Forward sweep fuses preconditioning, Gauss step and l_solve row by row
    // (the reference's values are row-local, so the interleaving is exact);
    // temporaries: A <- scaled upper band, C <- final diagonal, B <- l_solve result.
    const int n = nk;
    double up_prev = 0, dg_prev = 1, yy_prev = 0;
    for (int i = 0; i < n; i++) {
        double lo = 0, dg, up = 0, r;
        if (i == 0) { dg = 2.0; up = 0.0; r = 0.0; }
        else if (i == n - 1) { dg = 2.0; lo = 0.0; r = 0.0; }
        else {
            const double xm = sl.x(i - 1), x0 = sl.x(i), xp = sl.x(i + 1);
            const double ym = sl.y(i - 1), y0 = sl.y(i), yp = sl.y(i + 1);
            lo = 1.0 / 3.0 * (x0 - xm);
            dg = 2.0 / 3.0 * (xp - xm);
            up = 1.0 / 3.0 * (xp - x0);
            r = (yp - y0) / (xp - x0) - (y0 - ym) / (x0 - xm);
        }
        const double sd = 1.0 / dg;                                     // saved_diag
        lo *= sd;
        up *= sd;
        dg = 1.0;
        double sum = 0;
        if (i > 0) {
            const double xx = -lo / dg_prev;                            // Gauss step k = i-1
            lo = -xx;
            dg = dg + xx * up_prev;
            sum += lo * yy_prev;                                        // l_solve
        }
        const double yy = (r * sd) - sum;
        sl.a(i) = up; sl.c(i) = dg; sl.b(i) = yy;
        up_prev = up; dg_prev = dg; yy_prev = yy;
    }
    double bb_next = 0;
    for (int i = n - 1; i >= 0; i--) {                                  // r_solve
        double sum = 0;
        if (i < n - 1) sum += sl.a(i) * bb_next;
        const double bb = (sl.b(i) - sum) / sl.c(i);
        sl.b(i) = bb;
        bb_next = bb;
    }
    for (int i = 0; i < n - 1; i++) {                                   // spline.h:345-349
        const double dx = sl.x(i + 1) - sl.x(i);
        sl.a(i) = 1.0 / 3.0 * (sl.b(i + 1) - sl.b(i)) / dx;
        sl.c(i) = (sl.y(i + 1) - sl.y(i)) / dx - 1.0 / 3.0 * (2.0 * sl.b(i) + sl.b(i + 1)) * dx;
    }
    const double h = sl.x(n - 1) - sl.x(n - 2);                         // spline.h:367-370
    sl.a(n - 1) = 0.0;
    sl.c(n - 1) = 3.0 * sl.a(n - 2) * h * h + 2.0 * sl.b(n - 2) * h + sl.c(n - 2);
}

// ------------------------------------------------------------------------------------------------
// Phase A by a team of TS threads per slot (k_cand): setup_lane's arithmetic, element for element,
// with its point- and row-local parts spread over the team and only the two band sweeps serial:
//   A1 (team)  previous-path knots; control point k: its own Map::get_lane_pos call (the reference
//              makes one call per point, :744-768) -> global xy in a(npk+1+k)/b(npk+1+k), ok in
//              c(npk+1+k), local xy in x/y(npk+1+k);
//   A2 (r = 0) the distance rule over the control points (:762), knot truncation, fallback, meta;
//   A3 (team)  each band row's preconditioned terms: a = up/dg, c = lo/dg, b = rhs/dg;
//   A4 (r = 0) Gauss + l_solve forward, r_solve backward (one division per row each way);
//   A5 (team)  the segment coefficients (spline.h:345-349) and the last row (:367-370).
// The caller puts a block barrier between the steps.
// ------------------------------------------------------------------------------------------------
struct LaneGeom {
    int K, npk, ref_wp;
    double pos_x, pos_y, ca, sa, dist, min_cpd, ratio, ego_d;
};
// (from the K1 values it reads: the build's start pose and rotation, the ego's Frenet state)
__device__ __forceinline__ LaneGeom lane_geom_from(int K, double pos_x, double pos_y, double ca_m, double sa_m,
                                                   int ref_wp, double ratio_L, double ego_d, double start,
                                                   double ego_vd, int L) {
    LaneGeom g;
    g.K = K;
    g.npk = g.K > 0 ? g.K - 1 : 0;
    g.pos_x = pos_x; g.pos_y = pos_y;
    g.ca = ca_m; g.sa = sa_m;
    g.ref_wp = ref_wp;
    g.ratio = ratio_L;
    g.ego_d = ego_d;
    double min_cpd = start * 1;
    g.min_cpd = s_max(min_cpd, 5.0);
    const double d_diff = lane_offset(L) - g.ego_d;
    const double d_acc = 4;
    bool slow = false;
    double lst = 2.0;
    if ((ego_vd < 0) == (d_diff < 0)) {
        const double dmax = ego_vd * ego_vd / d_acc / 2;
        if (dmax > fabs(d_diff)) { slow = true; lst = fabs(ego_vd) / d_acc; }
    }
    if (!slow) {
        double rel = ego_vd;
        if (d_diff < 0) rel *= -1;
        const double add = fabs(d_diff);
        const double peak = sqrt(add * d_acc + rel * rel / 2);
        lst = (peak * 2 - rel) / d_acc;
    }
    double dist = start * lst;
    if (dist < 10.0) dist = 10.0;
    if (dist > 50) dist = 50;
    g.dist = dist;
    return g;
}
__device__ __forceinline__ LaneGeom lane_geom(const PrepV& pv, int64_t v, int64_t Sv, int L) {
    return lane_geom_from(pv.K[v], pv.pos_x[v], pv.pos_y[v], pv.ca_m[v], pv.sa_m[v], pv.ref_wp[v],
                          pv.ratio[L * Sv + v], pv.ego_d[v], pv.ego_speed[v], pv.ego_vd[v], L);
}

__device__ void team_a1(const MapV& m, const pp_scene_batch& in, const LaneGeom& g, int64_t s, int L,
                        const Slot& sl, int r, int TS) {
    const int64_t S = in.n_scenes;
    for (int i = r; i < g.npk; i += TS) {
        const double tx0 = in.prev_x[(int64_t)i * S + s] - g.pos_x;
        const double ty0 = in.prev_y[(int64_t)i * S + s] - g.pos_y;
        sl.x(i) = tx0 * g.ca - ty0 * g.sa;
        sl.y(i) = tx0 * g.sa + ty0 * g.ca;
    }
    if (r == 0) {
        sl.x(g.npk) = (g.pos_x - g.pos_x) * g.ca - (g.pos_y - g.pos_y) * g.sa;
        sl.y(g.npk) = (g.pos_x - g.pos_x) * g.sa + (g.pos_y - g.pos_y) * g.ca;
    }
    for (int k = r; k < 5; k += TS) {
        double cps = g.dist;
        for (int i = 1; i <= k; i++) cps = cps + g.min_cpd;
        double px, py;
        bool ok;
        if (cps > 0) get_lane_pos_fwd<kWalkPf>(m, g.ref_wp, g.ratio, cps, L, px, py, ok);
        else get_lane_pos(m, g.ref_wp, g.ratio, cps, L, px, py, ok);
        const int j = g.npk + 1 + k;
        sl.a(j) = px; sl.b(j) = py; sl.c(j) = ok ? 1.0 : 0.0;
        const double tx0 = px - g.pos_x, ty0 = py - g.pos_y;
        sl.x(j) = tx0 * g.ca - ty0 * g.sa;
        sl.y(j) = tx0 * g.sa + ty0 * g.ca;
    }
}

__device__ void team_a2(const LaneGeom& g, const Slot& sl) {
    int flags = 0;
    double lx = g.pos_x, ly = g.pos_y, total = 0;
    int ncp = 1;
    for (int i = 0; i < 5; i++) {
        const int j = g.npk + 1 + i;
        const double npx = sl.a(j), npy = sl.b(j);
        if (sl.c(j) == 0.0) flags |= kMetaWalkFail;
        total += sqrt((npx - lx) * (npx - lx) + (npy - ly) * (npy - ly));
        lx = npx; ly = npy;
        ncp++;
        if (total > 50 && ncp > 2) break;
    }
    int nk = g.npk + ncp;
    for (int i = 1; i < nk; i++) {                                      // :833-843
        if (sl.x(i) <= sl.x(i - 1)) { nk = i; flags |= kMetaTrunc; break; }
    }
    const bool fallback = nk < 3 || nk <= g.npk || fabs(g.ego_d) > 20;  // :848
    if (fallback) flags |= kMetaFallback;
    sl.m(0) = nk; sl.m(1) = ncp; sl.m(2) = g.npk; sl.m(3) = flags;
}

// Each team lane takes a contiguous run of rows, so the slope (y(i+1) - y(i)) / (x(i+1) - x(i))
// that row i's right-hand side shares with row i+1 is divided once per run, not twice.
__device__ void team_a3(const Slot& sl, int r, int TS) {
    if (sl.m(3) & kMetaFallback) return;
    const int n = sl.m(0);
    const int per = (n + TS - 1) / TS;
    const int i0 = r * per, i1 = i0 + per < n ? i0 + per : n;
    double sl_prev = 0;                                                 // slope of segment i-1
    if (i0 > 0 && i0 < n - 1) sl_prev = (sl.y(i0) - sl.y(i0 - 1)) / (sl.x(i0) - sl.x(i0 - 1));
    for (int i = i0; i < i1; i++) {
        double lo = 0, dg, up = 0, rr;
        if (i == 0) { dg = 2.0; up = 0.0; rr = 0.0; }
        else if (i == n - 1) { dg = 2.0; lo = 0.0; rr = 0.0; }
        else {
            const double xm = sl.x(i - 1), x0 = sl.x(i), xp = sl.x(i + 1);
            const double y0 = sl.y(i), yp = sl.y(i + 1);
            lo = 1.0 / 3.0 * (x0 - xm);
            dg = 2.0 / 3.0 * (xp - xm);
            up = 1.0 / 3.0 * (xp - x0);
            const double sl_i = (yp - y0) / (xp - x0);
            rr = sl_i - sl_prev;                // (yp - y0)/(xp - x0) - (y0 - ym)/(x0 - xm)
            sl_prev = sl_i;
        }
        if (i == 0 && n > 2) sl_prev = (sl.y(1) - sl.y(0)) / (sl.x(1) - sl.x(0));
        const double sd = 1.0 / dg;                                     // saved_diag
        sl.a(i) = up * sd; sl.c(i) = lo * sd; sl.b(i) = rr * sd;
    }
}

__device__ void team_a4(const Slot& sl) {
    if (sl.m(3) & kMetaFallback) return;
    const int n = sl.m(0);
    double up_prev = 0, dg_prev = 1, yy_prev = 0;
    for (int i = 0; i < n; i++) {
        double lo = sl.c(i);
        const double up = sl.a(i);
        double dg = 1.0;
        double sum = 0;
        if (i > 0) {
            const double xx = -lo / dg_prev;                            // Gauss step k = i-1
            lo = -xx;
            dg = dg + xx * up_prev;
            sum += lo * yy_prev;                                        // l_solve
        }
        const double yy = sl.b(i) - sum;
        sl.c(i) = dg; sl.b(i) = yy;
        up_prev = up; dg_prev = dg; yy_prev = yy;
    }
    double bb_next = 0;
    for (int i = n - 1; i >= 0; i--) {                                  // r_solve
        double sum = 0;
        if (i < n - 1) sum += sl.a(i) * bb_next;
        const double bb = (sl.b(i) - sum) / sl.c(i);
        sl.b(i) = bb;
        bb_next = bb;
    }
}

__device__ void team_a5(const Slot& sl, int r, int TS) {
    if (sl.m(3) & kMetaFallback) return;
    const int n = sl.m(0);
    for (int i = r; i < n - 1; i += TS) {                               // spline.h:345-349
        const double dx = sl.x(i + 1) - sl.x(i);
        const double a = 1.0 / 3.0 * (sl.b(i + 1) - sl.b(i)) / dx;
        const double c = (sl.y(i + 1) - sl.y(i)) / dx - 1.0 / 3.0 * (2.0 * sl.b(i) + sl.b(i + 1)) * dx;
        sl.a(i) = a; sl.c(i) = c;
        if (i == n - 2) {                                               // spline.h:367-370
            const double h = sl.x(n - 1) - sl.x(n - 2);
            sl.a(n - 1) = 0.0;
            sl.c(n - 1) = 3.0 * a * h * h + 2.0 * sl.b(n - 2) * h + c;
        }
    }
}
