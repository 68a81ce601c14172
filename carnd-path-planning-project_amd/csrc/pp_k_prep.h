// pp_k_prep.h — device: K0 and K1, scene preparation (src/main.cpp:1233-1438): ego derivation, Frenet
// frame, car matching, LaneChangePlanner, follow cars and LimitSpeed per candidate lane. k_sort_cars,
// k_prep (one lane per evaluation) and k_prep_g2..16 (G lanes per evaluation).
// Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// K1: scene preparation
// ------------------------------------------------------------------------------------------------
// k_cand groups (SPB scenes per group, or BPS groups per scene): k_prep marks the groups holding a
// kLimSlow scene in this bitmap for k_cand<true>
// (list/count: the flagged groups in the order k_prep found them, for k_cand<true>; count is zeroed
// before every K1)
// (BPS < 0: the flat all-paths geometry, groups of 256 consecutive candidates of the batch, C per
// scene: a scene lies in groups s C / 256 ... ((s + 1) C - 1) / 256)
struct GroupBits { uint32_t* bits; int SPB, BPS; uint32_t* list; uint32_t* count; int pose_by_wave; int C; };
// ---- K1 building blocks, shared by k_prep (one lane per evaluation) and k_prep_g2..16 (G lanes) ----

// Ego state of one evaluation: derivation (src/main.cpp:1233-1292), Frenet frame and ego matching
// (:1299-1320).
struct EgoSt {
    double ego_x, ego_y, yaw, ego_speed, ego_acc, esv_x, esv_y, dt0, p8x, p8y;
    double ego_s, ego_d, ego_vs, ego_vd, ratio[NL];
    int K, ref_wp, ego_lane;
    uint32_t status;
};

// G > 1: the G lanes of a group (this one is lane r) split the reference-waypoint scan; every
// lane ends with the same state
template <int G>
__device__ __forceinline__ void prep_ego(const MapV& m, const pp_scene_batch& in, const pp_params& P,
                                         int64_t S, int64_t s, int r, EgoSt& e) {
    e.status = 0;
    e.ego_x = in.ego_x[s]; e.ego_y = in.ego_y[s];
    e.yaw = in.ego_yaw_deg[s];
    double ego_speed = in.ego_speed_mph[s];
    ego_speed /= 2.237;
    e.ego_acc = 0; e.esv_x = 0; e.esv_y = 0; e.dt0 = 0;
    e.K = 0;
    e.p8x = 0; e.p8y = 0;
    // (the kept points are loaded with n_prev, not after it: rows 7-9 always exist, and a frame's
    // K1 would otherwise wait for two memory round trips in a row)
    const int np = in.n_prev[s];
    const double p7x = in.prev_x[7 * S + s], p7y = in.prev_y[7 * S + s];
    const double p8x = in.prev_x[8 * S + s], p8y = in.prev_y[8 * S + s];
    const double p9x = in.prev_x[9 * S + s], p9y = in.prev_y[9 * S + s];
    if (np >= PP_PREV_KEEP) {
        e.K = PP_PREV_KEEP;
        e.p8x = p8x; e.p8y = p8y;
        const double ax = e.p8x - p7x, ay = e.p8y - p7y;
        const double v2 = sqrt(ax * ax + ay * ay);
        e.esv_x = p9x - e.p8x; e.esv_y = p9y - e.p8y;
        const double v3 = sqrt(e.esv_x * e.esv_x + e.esv_y * e.esv_y);
        e.ego_acc = (v3 - v2) * 50;
        ego_speed = v3 * 50;
        e.esv_x *= 50; e.esv_y *= 50;
        e.ego_x = p9x; e.ego_y = p9y;
        e.dt0 = PP_PREV_KEEP / 50.0;
    }
    e.ego_speed = ego_speed;
    if (G == 1) init_reference_waypoint(m, e.ego_x, e.ego_y, e.ref_wp, e.ratio);
    else init_reference_waypoint_grp<G>(m, e.ego_x, e.ego_y, r, e.ref_wp, e.ratio);
    e.ego_s = 0; e.ego_d = 0;
    e.ego_lane = 0;
    int nwp_unused = 0;
    if (!lane_match(m, e.ref_wp, e.ratio, e.ego_x, e.ego_y, e.ego_s, e.ego_d, e.ego_lane, nwp_unused)) {
        e.ego_s = e.ego_d = 0;
        e.ego_lane = 0;
        e.status |= PP_ST_EGO_UNMATCHED;
    }
    project_speed(m, e.esv_x, e.esv_y, e.ref_wp, e.ego_vs, e.ego_vd);
    if (e.ego_acc > P.maximum_acc) e.ego_acc = P.maximum_acc;
    if (e.ego_acc < -P.maximum_acc) e.ego_acc = -P.maximum_acc;
}

// LaneChangePlanner's accumulation (src/main.cpp:377-445) and the follow-car selection
// (:1388-1410): order-dependent reductions over one car sequence. Every one is a minimum with ties
// to the lower iteration index (or an AND / a count), so a visiting order other than ascending
// ids gives the reference's result once ties compare that index explicitly — except for a chosen
// car whose id is the reference's 'no car' sentinel -1, which any later car replaces: such
// scenes (and car tables) are visited in iteration order.
// (Per-lane state is indexed by the car's lane through selects, sel/put: a dynamically indexed
// member array would live in scratch memory.)
// (each element passes an empty asm first: a select chain over the array's own elements is
// folded back into an indexed load, which puts the array in scratch memory)
template <typename T>
__device__ __forceinline__ T sel(const T (&a)[NL], int l) {
    T x = a[0];
    asm("" : "+v"(x));
#pragma unroll
    for (int i = 1; i < NL; i++) {
        T ai = a[i];
        asm("" : "+v"(ai));
        x = l == i ? ai : x;
    }
    return x;
}
template <typename T>
__device__ __forceinline__ void put(T (&a)[NL], int l, T x) {
#pragma unroll
    for (int i = 0; i < NL; i++) a[i] = l == i ? x : a[i];
}
// OR / sum over the G lanes of a group; (key, index) minimum with ties to the lower index
template <int G>
__device__ __forceinline__ uint32_t grp_or(uint32_t x) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) x |= (uint32_t)__shfl_xor((int)x, o, G);
    return x;
}
template <int G>
__device__ __forceinline__ uint32_t grp_sum(uint32_t x) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, G);
    return x;
}
template <int G>
__device__ __forceinline__ void grp_argmin(double& key, int& idx) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) {
        const double ok = __shfl_xor(key, o, G);
        const int oi = __shfl_xor(idx, o, G);
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
}
struct PlanAcc {
    int lane_speed[NL];                     // the int-truncated lane speed where bit l of ls_set
    int ls_set;                             // (else P.max_speed)
    double next_s[NL];
    int open_m;                             // lane_open, bit l
    int in_id; double in_s;
    int t_id[NL];
    double t_s[NL];
    // iteration index of each running minimum, kItBits each: next_s[l] at field l, the target-lane
    // car of lane l at field NL + l, the in-lane car at field 2 NL (the follow cars' velocities are
    // re-read from that index after the pass)
    static constexpr int kItBits = 64 / (2 * NL + 1);
    static constexpr uint64_t kItMask = (1ull << kItBits) - 1;
    uint64_t its;
    int nmatched;
    __device__ __forceinline__ int it_of(int f) const { return (int)((its >> (kItBits * f)) & kItMask); }
    __device__ __forceinline__ void set_it(int f, int it) {
        its = (its & ~(kItMask << (kItBits * f))) | ((uint64_t)it << (kItBits * f));
    }
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int l = 0; l < NL; l++) {
            lane_speed[l] = 0; next_s[l] = 1000;
            t_id[l] = -1; t_s[l] = 0;
        }
        open_m = (1 << NL) - 1;
        ls_set = 0; in_id = -1; in_s = 0; its = 0; nmatched = 0;
    }
    // one matched car (iteration index it) with its Frenet state
    __device__ __forceinline__ void add(const pp_params& P, const EgoSt& e, int T_in, int it, int id,
                                        double cs, double cd, int clane, double cvs, double cvd) {
        const double ego_s = e.ego_s, ego_vs = e.ego_vs, dt0 = e.dt0;
        nmatched++;
        // planner (src/main.cpp:379-444)
        const double sp = cs + cvs * dt0;
        if (sp > ego_s) {
            // the first car (in iteration order) with the smallest sp sets next_s; lane_speed
            // comes from it if it is within 200 m (an earlier, larger minimum never is then)
            // (next_s == 1000: still the initial value, which no car can set, so it wins the tie)
            const double ns = sel(next_s, clane);
            if (sp < ns || (sp == ns && ns != 1000 && it < it_of(clane))) {
                put(next_s, clane, sp);
                set_it(clane, it);
                set_speed(P, ego_s, clane, sp, cvs);
            }
        }
        bool open = true;
        double add = 2;
        if (T_in == clane) add = 0;
        const double min_dist = P.car_length + P.safety_distance + add;
        if (fabs(ego_s - sp) < min_dist) open = false;
        if (sp > ego_s && cvs < ego_vs) {
            const double car_dist = sp - ego_s - P.car_length - P.safety_distance - add;
            const double sd = ego_vs - cvs;
            const double dtm = sd / P.relaxed_acc;
            const double ddist = ego_vs * dtm - sd / 2 * dtm;
            if (car_dist < ddist) open = false;
        }
        if (sp < ego_s && cvs > ego_vs && sp + 50 > ego_s) {
            const double car_dist = ego_s - sp - P.car_length - P.safety_distance - add;
            const double sd = cvs - ego_vs;
            double dtm = sd / P.relaxed_acc;
            if (T_in == e.ego_lane) dtm += 2;
            const double md = sd * dtm;
            if (car_dist < md) open = false;
        }
        if (!open) open_m &= ~(1 << clane);
        // follow cars (src/main.cpp:1391-1409); the target-lane choice for every candidate lane
        const double s0 = cs + cvs * dt0;
        const double d0 = cd + cvd * dt0;
        if (s0 > ego_s && fabs(d0 - e.ego_d) < 3) {
            if (in_id == -1 || in_s > s0 || (in_s == s0 && it < it_of(2 * NL))) {
                in_id = id; in_s = s0; set_it(2 * NL, it);
            }
        }
#pragma unroll
        for (int L = 0; L < NL; L++) {
            if (s0 >= ego_s - P.car_length - P.safety_distance && fabs(d0 - lane_offset(L)) < 3) {
                if (t_id[L] == -1 || t_s[L] > s0 || (t_s[L] == s0 && it < it_of(NL + L))) {
                    t_id[L] = id; t_s[L] = s0; set_it(NL + L, it);
                }
            }
        }
    }
    // the lane's speed where car (sp, cvs) holds next_s of its lane (src/main.cpp:385-399)
    __device__ __forceinline__ void set_speed(const pp_params& P, double ego_s, int l, double sp, double cvs) {
        if (sp - ego_s < 200) {
            int speed = (int)cvs;
            if (speed > P.max_speed) speed = (int)P.max_speed;
            if (sp - ego_s > 100)
                speed = (int)(speed + (P.max_speed - speed) * (sp - ego_s - 100) / (200.0 - 100.0));
            put(lane_speed, l, speed);
            ls_set |= 1 << l;
        } else {
            ls_set &= ~(1 << l);
        }
    }
    // G cars at once, one per lane of the group (car it = this lane's iteration index; valid: a
    // matched car), all with iteration indices above every car added before: the same state as
    // add() over them in iteration order. Every selection is a minimum of (key, iteration index),
    // reduced over the group by shuffles and merged into the running one by add()'s own rule; the
    // per-car terms (planner keys, lane_open) are computed by each lane for its own car. The
    // caller keeps add() for groups holding a car whose id is the 'no car' sentinel -1, which
    // add() lets any later car replace.
    template <int G>
    __device__ __forceinline__ void add_group(const pp_params& P, const EgoSt& e, int T_in, bool valid, int it,
                                              int id, double cs, double cd, int clane, double cvs, double cvd) {
        const double ego_s = e.ego_s, ego_vs = e.ego_vs, dt0 = e.dt0;
        const double kInf = __builtin_inf();
        constexpr int kNone = 0x7fffffff;
        nmatched += (int)grp_sum<G>(valid ? 1u : 0u);
        const double sp = cs + cvs * dt0;
        // next_s per lane: the first car with the smallest sp in (ego_s, 1000)
#pragma unroll
        for (int l = 0; l < NL; l++) {
            double k = valid && clane == l && sp > ego_s && sp < 1000 ? sp : kInf;
            int ki = k == kInf ? kNone : it;
            grp_argmin<G>(k, ki);
            const double wcvs = __shfl(cvs, ki == kNone ? 0 : ki - (it - (int)(threadIdx.x % G)), G);
            const double ns = sel(next_s, l);
            if (ki != kNone && (k < ns || (k == ns && ns != 1000 && ki < it_of(l)))) {
                put(next_s, l, k);
                set_it(l, ki);
                set_speed(P, ego_s, l, k, wcvs);
            }
        }
        // lane_open (src/main.cpp:401-444): a lane closes if any of its cars closes it
        bool open = true;
        {
            double add = 2;
            if (T_in == clane) add = 0;
            const double min_dist = P.car_length + P.safety_distance + add;
            if (fabs(ego_s - sp) < min_dist) open = false;
            if (sp > ego_s && cvs < ego_vs) {
                const double car_dist = sp - ego_s - P.car_length - P.safety_distance - add;
                const double sd = ego_vs - cvs;
                const double dtm = sd / P.relaxed_acc;
                const double ddist = ego_vs * dtm - sd / 2 * dtm;
                if (car_dist < ddist) open = false;
            }
            if (sp < ego_s && cvs > ego_vs && sp + 50 > ego_s) {
                const double car_dist = ego_s - sp - P.car_length - P.safety_distance - add;
                const double sd = cvs - ego_vs;
                double dtm = sd / P.relaxed_acc;
                if (T_in == e.ego_lane) dtm += 2;
                const double md = sd * dtm;
                if (car_dist < md) open = false;
            }
        }
        open_m &= ~(int)grp_or<G>(valid && !open ? 1u << clane : 0u);
        // follow cars (src/main.cpp:1391-1409): the in-lane car, the target-lane car of each lane
        const double s0 = cs + cvs * dt0;
        const double d0 = cd + cvd * dt0;
        const int r0 = (int)(threadIdx.x % G), itb = it - r0;    // the group's first iteration index
        {
            double k = valid && s0 > ego_s && fabs(d0 - e.ego_d) < 3 ? s0 : kInf;
            int ki = valid && s0 > ego_s && fabs(d0 - e.ego_d) < 3 ? it : kNone;
            grp_argmin<G>(k, ki);
            const int wid = __shfl(id, ki == kNone ? 0 : ki - itb, G);
            if (ki != kNone && (in_id == -1 || in_s > k || (in_s == k && ki < it_of(2 * NL)))) {
                in_id = wid; in_s = k; set_it(2 * NL, ki);
            }
        }
#pragma unroll
        for (int L = 0; L < NL; L++) {
            const bool q = valid && s0 >= ego_s - P.car_length - P.safety_distance && fabs(d0 - lane_offset(L)) < 3;
            double k = q ? s0 : kInf;
            int ki = q ? it : kNone;
            grp_argmin<G>(k, ki);
            const int wid = __shfl(id, ki == kNone ? 0 : ki - itb, G);
            if (ki != kNone && (t_id[L] == -1 || t_s[L] > k || (t_s[L] == k && ki < it_of(NL + L)))) {
                t_id[L] = wid; t_s[L] = k; set_it(NL + L, ki);
            }
        }
    }
};


// TrajectoryBuilder::build start pose (src/main.cpp:583-610): the last kept previous point and the
// heading of the last kept step, or the ego pose
__device__ __forceinline__ void start_pose(const pp_scene_batch& in, int64_t S, int64_t s, const EgoSt& e,
                                           double& pos_x, double& pos_y, double& angle) {
    if (e.K == 0) {
        pos_x = e.ego_x; pos_y = e.ego_y;
        angle = e.yaw * kPi / 180;
    } else {
        pos_x = in.prev_x[9 * S + s]; pos_y = in.prev_y[9 * S + s];
        const double vx = pos_x - e.p8x, vy = pos_y - e.p8y;
        if (vx * vx + vy * vy < kEps) angle = e.yaw * kPi / 180;
        else angle = ppg::atan2(pos_y - e.p8y, pos_x - e.p8x);       // glibc's atan2, bit for bit
    }
}
// The frame's rotations tv = cos(-a), sin(-a), cos(a), sin(a) as the reference's libm computes
// them. glibc's sin is odd and its cos even bit for bit (both reduce |x| and apply the sign last;
// tests/test_glibcm.py checks the restatement on 3.9 M arguments), so two evaluations give all
// four: cos(-a) = cos(a), sin(-a) = -sin(a). G > 1: lane r of the group computes tv[r] (r < 4;
// the others hold nothing), except when the restated reduction fails (every lane then holds all
// four, from the library's own reduction)
template <int G>
__device__ __forceinline__ void frame_trig(double angle, int r, double tv[4]) {
    bool tfail = false;
    if (G == 1) {
        tfail = !ppg::cos(angle, tv[2]);
        tfail |= !ppg::sin(angle, tv[3]);
        tv[0] = tv[2];
        tv[1] = -tv[3];
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t % G != r) continue;
            double v;
            tfail |= !((t & 1) ? ppg::sin(angle, v) : ppg::cos(angle, v));
            tv[t] = t == 1 ? -v : v;
        }
    }
    if (G > 1) tfail = grp_or<G>(tfail ? 1u : 0u) != 0u;
    if (tfail) {                              // every lane: both pairs (rare)
        double sm, cm, sp, cp;
        ppm::sincos_pp<true>(-angle, sm, cm);
        ppm::sincos_pp<true>(angle, sp, cp);
        tv[0] = cm; tv[1] = sm; tv[2] = cp; tv[3] = sp;
    }
}

// The rest of K1 after the car pass (src/main.cpp:447-484, 1358-1438, 583-610, 786-823): scores
// and the target lane, LimitSpeed for the in-lane car (task 0) and each lane's target car (task
// 1 + L), k_cand<false>'s range checks, the build start pose and the frame rotations (tasks 0-3:
// cos(-a), sin(-a), cos(a), sin(a)). G > 1: the tasks are spread over the lanes of the group
// (lane r takes tasks r, r + G, ...) and lane 0 writes the scene's record.
template <int G>
__device__ __forceinline__ void prep_finish(const pp_scene_batch& in, const pp_params& P, const PrepV& pv,
                                            pp_scene_info* info, uint32_t* out_status, const GroupBits& gb,
                                            int64_t S, int64_t Sv, int64_t s, int64_t v, int draw, bool tab,
                                            int r, int T_in, const EgoSt& e, const PlanAcc& a,
                                            uint32_t status) {
    // scores + argmax (src/main.cpp:447-484)
    int best_lane = e.ego_lane;
    double best_score = 0;
    double score[NL];
#pragma unroll
    for (int lane = 0; lane < NL; lane++) {
        score[lane] = 0;
        if (lane != e.ego_lane && !((a.open_m >> lane) & 1)) continue;
        const double lsp = ((a.ls_set >> lane) & 1) ? (double)a.lane_speed[lane] : P.max_speed;
        const double speed_score = s_min(lsp / P.max_speed, 1.0);
        const double distance_score = 1 - fabs((double)(T_in - lane)) / 2;
        const double free_score = s_min(1.0, a.next_s[lane] / 100);
        const double total = speed_score + distance_score / 2 + free_score;
        score[lane] = total;
        if (total > best_score) { best_score = total; best_lane = lane; }
    }
    int T;
    if (abs(e.ego_lane - best_lane) > 1) {
        const int nl = best_lane > e.ego_lane ? e.ego_lane + 1 : e.ego_lane - 1;
        T = ((a.open_m >> nl) & 1) ? nl : e.ego_lane;
        status |= PP_ST_JUMP_RULE;
    } else {
        T = best_lane;
    }
    const int open_mask = a.open_m;
    if (open_mask != (1 << NL) - 1) status |= PP_ST_LANE_CLOSED;
    if (T != e.ego_lane) {                                             // src/main.cpp:1358-1369
        const double dtl = lane_offset(T);
        const double diff = fabs(e.ego_vd * 1.0 + e.ego_d - dtl);
        if (diff > 6.0) { T = e.ego_lane; status |= PP_ST_TOO_FAR; }
    }
    // LimitSpeed for the in-lane car and the per-lane target car (src/main.cpp:1411-1438); the
    // reference's "no car" is id -1 (:1383-1432): a chosen car whose id is -1 reads as none; ids
    // are what :1411 compares. k_cand<false> divides by reciprocals without range checks: every
    // speed and ramp time of the scene must be in range (else kLimSlow)
    int lim_mask = 0;
    bool ok = true;
    for (int t = r; t < 1 + NL; t += G) {
        bool has = a.in_id != -1, in_lane = true;
        double fs = a.in_s;
        int fit = a.it_of(2 * NL);
#pragma unroll
        for (int L = 0; L < NL; L++)
            if (t == 1 + L) { has = a.t_id[L] != -1 && a.t_id[L] != a.in_id; in_lane = false; fs = a.t_s[L]; fit = a.it_of(NL + L); }
        if (!has) continue;
        double ts, tt, fvx, fvy;
        bool col;
        car_velocity(in, P, S, s, draw, tab, fit, fvx, fvy);
        const int code = limit_speed(P, fvx, fvy, fs, e.ego_s, e.ego_speed, e.ego_acc, in_lane, ts, tt, col);
        status |= limit_flag(code) | (col ? PP_ST_COLLISION : 0u);
        if (t == 0) { pv.in_ts[v] = ts; pv.in_tt[v] = tt; }
        else { pv.l_ts[(t - 1) * Sv + v] = ts; pv.l_tt[(t - 1) * Sv + v] = tt; }
        lim_mask |= 1 << t;
        ok = ok && speed_in_range(ts) && speed_in_range(tt);
    }
    for (int k = r; k < P.n_speeds; k += G) {
        const double vk = cand_speed(P, e.ego_speed, k);
        ok = ok && speed_in_range(vk) && speed_in_range(fabs(e.ego_speed - vk) / P.relaxed_acc);
    }
    ok = ok && speed_in_range(e.ego_speed);
    if (G > 1) {
        status = grp_or<G>(status);
        lim_mask = (int)grp_or<G>((uint32_t)lim_mask);
        ok = grp_or<G>(ok ? 0u : 1u) == 0u;
    }
    // TrajectoryBuilder::build start pose (src/main.cpp:583-610) + frame rotations (:786-823)
    // (gb.pose_by_wave: the wave step's phase-A waves compute and record the start pose, its
    // rotations and the heading's kLimSlow bit themselves, off K1's critical path)
    double pos_x = 0, pos_y = 0, angle = 0;
    if (!gb.pose_by_wave) {
        start_pose(in, S, s, e, pos_x, pos_y, angle);
        // heading beyond the hot loop's medium trig range (only from an absurd telemetry yaw): the
        // scene is evaluated by the k_cand<true> instantiation with the library's large reduction
        if (!(fabs(angle) <= kSlowAngle)) lim_mask |= kLimSlow;
    }
    if (!ok) lim_mask |= kLimSlow;
    if ((lim_mask & kLimSlow) && r == 0 && gb.bits) {   // (k_step_small: no bitmap)
        const int64_t g0 = gb.BPS == 1 ? s / gb.SPB : gb.BPS < 0 ? s * gb.C / 256 : s * gb.BPS;
        const int nb = gb.BPS < 0 ? (int)(((s + 1) * gb.C - 1) / 256 - g0 + 1) : gb.BPS;
        for (int b = 0; b < nb; b++) {
            const uint32_t bit = 1u << ((g0 + b) & 31);
            const uint32_t old = atomicOr(&gb.bits[(g0 + b) >> 5], bit);
            if (!(old & bit) && gb.list) gb.list[atomicAdd(gb.count, 1u)] = (uint32_t)(g0 + b);
        }
    }
    // the frame's rotations cos(-angle), sin(-angle) (:786-787) and cos(angle), sin(angle)
    // (:822-823) as the reference's libm computes them (pp_glibcm.h): every knot is a product with
    // them, so the spline and every path position carry their exact bits. Headings of 1e8 rad and
    // more (only from an absurd telemetry yaw) are outside the restated reduction.
    if (!gb.pose_by_wave) {
        double tv[4];
        frame_trig<G>(angle, r, tv);
        double* const tdst[4] = {pv.ca_m, pv.sa_m, pv.ca_p, pv.sa_p};
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (G == 1 || t % G == r) tdst[t][v] = tv[t];
        if (r == 0) { pv.pos_x[v] = pos_x; pv.pos_y[v] = pos_y; pv.angle[v] = angle; }
    }
    if (r != 0) return;
    pv.ego_speed[v] = e.ego_speed; pv.ego_d[v] = e.ego_d; pv.ego_vd[v] = e.ego_vd;
#pragma unroll
    for (int l = 0; l < NL; l++) { pv.ratio[l * Sv + v] = e.ratio[l]; pv.score[l * Sv + v] = score[l]; }
    pv.K[v] = e.K; pv.ref_wp[v] = e.ref_wp; pv.T[v] = T; pv.ego_lane[v] = e.ego_lane;
    pv.open_mask[v] = open_mask; pv.lim_mask[v] = lim_mask; pv.status[v] = status;
    if (draw == 0) out_status[s] = 0;        // k_cand ORs its flags in (atomics when a scene spans blocks)
    if (info && draw == 0) {
        pp_scene_info I = {};
        I.ego_x = e.ego_x; I.ego_y = e.ego_y; I.ego_speed = e.ego_speed; I.ego_acc = e.ego_acc;
        I.ego_s = e.ego_s; I.ego_d = e.ego_d; I.ego_vs = e.ego_vs; I.ego_vd = e.ego_vd;
        for (int l = 0; l < NL; l++) { I.ref_ratio[l] = e.ratio[l]; I.lane_score[l] = score[l]; }
        I.ref_wp = e.ref_wp; I.ego_lane = e.ego_lane; I.target_lane = T; I.lane_open_mask = open_mask;
        I.n_matched_cars = a.nmatched; I.in_lane_car = a.in_id;
        info[s] = I;
    }
}

// Monte-Carlo sensor noise on one car row (include/pp.h pp_params)
__device__ __forceinline__ void car_noise(const pp_params& P, int64_t s, int draw, int row, double& cx,
                                          double& cy, double& cvx, double& cvy) {
    const uint64_t gs = (uint64_t)(P.noise_first_scene + s);
    double g[4];
    ppsynth::mc_gauss4(P.noise_seed, gs, draw, row, g);      // (mc_gauss q = 0..3)
    cx += P.noise_pos_sigma * g[0];
    cy += P.noise_pos_sigma * g[1];
    cvx += P.noise_vel_sigma * g[2];
    cvy += P.noise_vel_sigma * g[3];
}

// kW4: the 4-waves-per-SIMD instantiation (<= 128 VGPRs): for batches whose wave count fills
// whole rounds of 4 waves per SIMD better than of 3 (prep_w4 in pp_launch.h)
constexpr int kSortDmax = 16;    // k_prep sorts a scene's rows nearest first below this many draws
// K0 (round 6; PP_DBG_SORT_CARS selects it per call): each scene's cars in k_prep's visiting order, visit-major.
// k_prep visits a scene's rows nearest first (below), and read them in that order straight from the
// batch's row-major arrays: a wave's load of visit k gathers 64 scenes' rows from up to 12 rows,
// each cache line partly used and fetched again at later visits (FETCH ~7x the scene record,
// DESIGN.md §4). k_sort_cars computes the same order (the same keys, the same network, the same
// identity-order rules) and writes the rows permuted into visit-major arrays x[k][s], ... through a
// per-lane LDS column, so k_prep's visit k reads 64 consecutive values per field. Only for batches
// without a car table, fewer than kSortDmax draws and at most 16 rows per scene (the host's
// condition); the values are copies, so k_prep's results are the same bits.
struct SortedCars {
    double *x, *y, *vx, *vy;      // [k][S], k < rows: the k-th visited row's fields
    int* id;                      // [k][S]
    uint64_t* order;              // [S]: the visiting order, one row index per nibble
    int rows;                     // min(car_stride, 16); 0: not in use
};
__device__ __forceinline__ uint64_t car_order(const pp_scene_batch& in, int64_t S, int64_t s, double ex,
                                              double ey, int iters) {
    uint64_t order = 0xFEDCBA9876543210ull;
    if (!(iters > 1 && iters <= 16)) return order;
    uint32_t key[16];
    bool neg = false;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        key[j] = 0xFFFFFFF0u | (uint32_t)j;
        if (j < iters) {
            const int64_t ix = (int64_t)j * S + s;
            const double dx = in.car_x[ix] - ex, dy = in.car_y[ix] - ey;
            const float f = (float)(dx * dx + dy * dy);
            key[j] = (__float_as_uint(f) & ~15u) | (uint32_t)j;
            neg |= in.car_id[ix] < 0;
        }
    }
#pragma unroll
    for (int pw = 1; pw < 16; pw <<= 1)
#pragma unroll
        for (int k = pw; k >= 1; k >>= 1)
#pragma unroll
            for (int j = k % pw; j < 16 - k; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; i++)
                    if ((i + j) / (2 * pw) == (i + j + k) / (2 * pw)) {
                        const uint32_t lo = key[i + j] < key[i + j + k] ? key[i + j] : key[i + j + k];
                        const uint32_t hi = key[i + j] < key[i + j + k] ? key[i + j + k] : key[i + j];
                        key[i + j] = lo; key[i + j + k] = hi;
                    }
    if (neg) return order;
    order = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) order |= (uint64_t)(key[j] & 15u) << (4 * j);
    return order;
}
__global__ __launch_bounds__(256) void k_sort_cars(pp_scene_batch in, SortedCars sc, int64_t s0, int64_t s1) {
    __shared__ double col[16 * 256];          // this lane's rows of one field: col[j * 256 + lane]
    const int64_t S = in.n_scenes;
    const int t = threadIdx.x;
    const int64_t s = s0 + (int64_t)blockIdx.x * 256 + t;
    if (s >= s1) return;                      // (no barrier below: every lane uses its own column)
    int iters = in.n_cars[s];
    if (iters > in.car_stride) iters = in.car_stride;
    // the ego position k_prep's keys use (prep_ego: the last kept point when 10 are kept)
    const int np = in.n_prev[s];
    const double ex = np >= PP_PREV_KEEP ? in.prev_x[9 * S + s] : in.ego_x[s];
    const double ey = np >= PP_PREV_KEEP ? in.prev_y[9 * S + s] : in.ego_y[s];
    const uint64_t order = car_order(in, S, s, ex, ey, iters);
    sc.order[s] = order;
    const double* src[4] = {in.car_x, in.car_y, in.car_vx, in.car_vy};
    double* dst[4] = {sc.x, sc.y, sc.vx, sc.vy};
#pragma unroll
    for (int f = 0; f < 4; f++) {
        for (int j = 0; j < iters; j++) col[j * 256 + t] = src[f][(int64_t)j * S + s];
        for (int k = 0; k < iters; k++) dst[f][(int64_t)k * S + s] = col[(int)((order >> (4 * k)) & 15) * 256 + t];
    }
    // the ids in the low half of this lane's own double slots (the waves of the block run without a
    // barrier: a lane must never touch another lane's slots)
    int* icol = (int*)col;
    for (int j = 0; j < iters; j++) icol[2 * (j * 256 + t)] = in.car_id[(int64_t)j * S + s];
    for (int k = 0; k < iters; k++) sc.id[(int64_t)k * S + s] = icol[2 * ((int)((order >> (4 * k)) & 15) * 256 + t)];
}

// kK0: k_sort_cars ran (srt holds the rows visit-major); a separate instantiation, so the default
// path carries no test of it
template <bool kLdsMap, bool kW4 = false, bool kK0 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kW4 ? 4 : kPrepWaves))) void k_prep(MapG mg, pp_scene_batch in, pp_params P, PrepV pv,
                                              pp_scene_info* info, uint32_t* out_status, GroupBits gb,
                                              int64_t v0, int64_t v1, SortedCars srt) {
    extern __shared__ __attribute__((aligned(16))) double smap[];
    const int n = mg.n;
#ifdef PP_TRACE
    if (threadIdx.x == 0 && blockIdx.x < (unsigned)(kTraceMax - kTraceK1)) {
        trace_at(kTraceK1 + blockIdx.x, 0);
        g_trace[8 * (kTraceK1 + blockIdx.x) + 7] = trace_hwid();
    }
#endif
    // the approach table: in LDS after the map (16-B aligned) in k_prep<true, false> (the host
    // sizes the launch for it, or passes none), else in global memory
    constexpr bool kAtabL = kLdsMap && !kW4;
    double* satab = smap + ((kMapArrays * n + 1) & ~1);
    if (kLdsMap) {
        stage_map(smap, mg.buf, kMapArrays * n);
        if (kAtabL && mg.atab) stage_map(satab, mg.atab, kAtabD * n);
        __syncthreads();
    }
#ifdef PP_TRACE
    if (threadIdx.x == 0 && blockIdx.x < (unsigned)(kTraceMax - kTraceK1)) trace_at(kTraceK1 + blockIdx.x, 1);
#endif
    MapV m = map_view(kLdsMap ? smap : mg.buf, n, mg.fastm);
    m.wg = mg.wg;                         // the closest-waypoint cell table (global memory)
    m.wseg = mg.wseg;                     // reference segment lengths and reciprocals (global memory)
    m.atab = kAtabL ? satab : mg.atab;    // the approach table (LDS or global memory)
    m.atab_on = mg.atab != nullptr;
    // one lane per evaluation v = s * D + d (scene s, Monte-Carlo draw d; D = 1 without noise):
    // inputs are read at scene s (stride S), the prep record is written at v (stride Sv)
    const int64_t S = in.n_scenes;
    const int D = P.n_draws > 1 ? P.n_draws : 1;
    const int64_t Sv = S * D;
    // evaluations [v0, v1) of the batch (pp_eval's chunked pipeline launches K1 per chunk)
    const int64_t v = v0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= v1 || v >= Sv) return;
    const int64_t s = D == 1 ? v : v / D;
    const int draw = (int)(v - s * D);

    EgoSt e;
    PP_REGION_K("ego");
    prep_ego<1>(m, in, P, S, s, 0, e);
    PP_REGION_K("sort");
    uint32_t status = e.status;
    const int T_in = in.prev_target_lane[s];
    PlanAcc a;
    a.init();
    int ncar = in.n_cars[s];
    if (ncar > in.car_stride) ncar = in.car_stride;
    // Without a car table: the frame's rows in order (ascending ids). With one (the reference's
    // persistent std::map): its tab_slots slots in order (ascending ids, include/pp.h), each car
    // either reported this frame (re-matched; slot overwritten, or erased when matching fails,
    // src/main.cpp:1329-1348) or taken from its stale slot.
    const bool tab = in.tab_valid != nullptr;
    const int iters = tab ? in.tab_slots : ncar;
    // Visiting order (PlanAcc: any order once ties compare the iteration index). Without a car
    // table the rows are visited nearest first (squared distance to the ego, a 4-bit row index in
    // the low mantissa bits of a float key, sorted by a Batcher network): the k-th visit of every
    // lane of a wave then walks a similar number of lane segments in lane_matching, which is where
    // the divergence was. With a table, or a negative car id (the reference's -1 'no car'
    // sentinel), the identity order is kept. (more than 16 rows: the identity order.) So do
    // Monte-Carlo batches of 16 draws or more: a wave's lanes are the draws of at most 4 scenes
    // (v = s D + d), which visit the same rows in lockstep anyway
    uint64_t order = 0xFEDCBA9876543210ull;
    bool sorted = false;
    // K0 ran (k_sort_cars): its order, and the rows in visit-major arrays
    constexpr bool k0 = kK0;
    if (k0) { order = srt.order[s]; sorted = true; }
    if (!k0 && !tab && iters > 1 && iters <= 16 && D < kSortDmax) {
        uint32_t key[16];
        bool neg = false;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            key[j] = 0xFFFFFFF0u | (uint32_t)j;
            if (j < iters) {
                const int64_t ix = (int64_t)j * S + s;
                const double dx = in.car_x[ix] - e.ego_x, dy = in.car_y[ix] - e.ego_y;
                const float f = (float)(dx * dx + dy * dy);
                key[j] = (__float_as_uint(f) & ~15u) | (uint32_t)j;
                neg |= in.car_id[ix] < 0;
            }
        }
#pragma unroll
        for (int pw = 1; pw < 16; pw <<= 1)
#pragma unroll
            for (int k = pw; k >= 1; k >>= 1)
#pragma unroll
                for (int j = k % pw; j < 16 - k; j += 2 * k)
#pragma unroll
                    for (int i = 0; i < k; i++)
                        if ((i + j) / (2 * pw) == (i + j + k) / (2 * pw)) {
                            const uint32_t lo = key[i + j] < key[i + j + k] ? key[i + j] : key[i + j + k];
                            const uint32_t hi = key[i + j] < key[i + j + k] ? key[i + j + k] : key[i + j];
                            key[i + j] = lo; key[i + j + k] = hi;
                        }
        if (!neg) {
            order = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) order |= (uint64_t)(key[j] & 15u) << (4 * j);
            sorted = true;
        }
    }
    static_assert(PP_MAX_CARS <= (1 << PlanAcc::kItBits), "iteration index fields");
    int p = 0;                              // next unread row (table mode)
    for (int kk = 0; kk < iters; kk++) {
        PP_REGION_K("carload");
        const int it = sorted ? (int)((order >> (4 * kk)) & 15) : kk;
        int row = it;
        const int64_t tix = (int64_t)it * S + s;
        // table mode: slot `it` holds car id sid (slots in ascending id order, include/pp.h)
        const int sid = tab ? (in.tab_id ? in.tab_id[tix] : it) : 0;
        if (tab) {
            while (p < ncar && in.car_id[(int64_t)p * S + s] < sid) p++;    // ids must ascend
            row = (p < ncar && in.car_id[(int64_t)p * S + s] == sid) ? p++ : -1;
        }
        int id;
        double cx, cy, cvx, cvy, cs, cd, cvs, cvd;
        int clane = 0;
        if (row >= 0) {
            if (k0) {                       // visit kk's row, visit-major (coalesced)
                const int64_t kx = (int64_t)kk * S + s;
                id = srt.id[kx];
                cx = srt.x[kx]; cy = srt.y[kx]; cvx = srt.vx[kx]; cvy = srt.vy[kx];
            } else {
                const int64_t ix = (int64_t)row * S + s;
                id = in.car_id[ix];
                cx = in.car_x[ix]; cy = in.car_y[ix]; cvx = in.car_vx[ix]; cvy = in.car_vy[ix];
            }
            if (draw > 0) car_noise(P, s, draw, row, cx, cy, cvx, cvy);
            int nwp = 0;
            PP_DIAGC(17, true);
            PP_REGION_K("match");
            if (!lane_match(m, e.ref_wp, e.ratio, cx, cy, cs, cd, clane, nwp)) {
                status |= PP_ST_CAR_UNMATCHED;
                if (tab) in.tab_valid[tix] = 0;
                continue;
            }
            PP_REGION_K("proj");
            project_speed(m, cvx, cvy, nwp, cvs, cvd);
            if (tab) {
                in.tab_valid[tix] = 1; in.tab_lane[tix] = clane;
                in.tab_s[tix] = cs; in.tab_d[tix] = cd; in.tab_vs[tix] = cvs; in.tab_vd[tix] = cvd;
                in.tab_vx[tix] = cvx; in.tab_vy[tix] = cvy;
            }
        } else {
            if (!in.tab_valid[tix]) continue;
            id = sid;
            clane = in.tab_lane[tix];
            cs = in.tab_s[tix]; cd = in.tab_d[tix]; cvs = in.tab_vs[tix]; cvd = in.tab_vd[tix];
        }
        PP_REGION_K("plan");
        a.add(P, e, T_in, it, id, cs, cd, clane, cvs, cvd);
    }
    PP_REGION_K("finish");
    prep_finish<1>(in, P, pv, info, out_status, gb, S, Sv, s, v, draw, tab, 0, T_in, e, a, status);
#ifdef PP_TRACE
    if ((threadIdx.x & 63) == 0 && blockIdx.x < (unsigned)(kTraceMax - kTraceK1))
        trace_at(kTraceK1 + blockIdx.x, 2 + (threadIdx.x >> 6));
#endif
}

// K1 for small batches: a group of G lanes per evaluation (G = 2 ... 16; kernels k_prep_g2 ... k_prep_g16), so that a batch of a few
// thousand scenes still fills the chip (BASELINE config 2: 4,096 scenes). Lane r of a group matches
// rows r, r + G, ... (coalesced across the group) and scans every G-th waypoint for the Frenet
// frame; the planner's pass then runs over each round's G cars in ascending row order on every
// lane of the group (the cars' Frenet states exchanged by lane shuffles), i.e. in the reference's
// own iteration order. With a car table the group's lanes take its slots the same way (slot r,
// r + G, ...; prep_grp_eval below): eval_plan never forces one lane per scene for table mode.
// One evaluation v by the G lanes of a group (this one is lane r); every lane of the group runs it
template <int G>
__device__ __forceinline__ void prep_grp_eval(const MapV& m, const pp_scene_batch& in, const pp_params& P,
                                              const PrepV& pv, pp_scene_info* info, uint32_t* out_status,
                                              const GroupBits& gb, int64_t v, int r) {
    const int64_t S = in.n_scenes;
    const int D = P.n_draws > 1 ? P.n_draws : 1;
    const int64_t Sv = S * D;
    const int64_t s = D == 1 ? v : v / D;
    const int draw = (int)(v - s * D);

    EgoSt e;
    PP_TRACE_K1(0);
    prep_ego<G>(m, in, P, S, s, r, e);
    PP_TRACE_K1(1);
    uint32_t status = e.status;
    const int T_in = in.prev_target_lane[s];
    PlanAcc a;
    a.init();
    // row r of the first G rows, loaded with n_cars rather than after it (rows below car_stride
    // exist; the frame's K1 waits for one memory round trip here, not two)
    int pid0 = 0;
    double px0 = 0, py0 = 0, pvx0 = 0, pvy0 = 0;
    if (r < in.car_stride) {
        const int64_t ix = (int64_t)r * S + s;
        pid0 = in.car_id[ix];
        px0 = in.car_x[ix]; py0 = in.car_y[ix]; pvx0 = in.car_vx[ix]; pvy0 = in.car_vy[ix];
    }
    int ncar = in.n_cars[s];
    if (ncar > in.car_stride) ncar = in.car_stride;
    // Without a car table: the frame's rows. With one (the reference's persistent std::map, as
    // k_prep): its tab_slots slots in order, each either reported this frame (re-matched; the slot
    // overwritten, or erased when matching fails, src/main.cpp:1329-1348) or taken from its stale
    // slot. Iteration index = row or slot, as in k_prep.
    const bool tab = in.tab_valid != nullptr;
    const int iters = tab ? in.tab_slots : ncar;
    uint32_t ust = 0;
    for (int j0 = 0; j0 < iters; j0 += G) {
        const int j = j0 + r;
        int okl = 0, id = 0;                  // okl: matched | lane << 1
        double cs = 0, cd = 0, cvs = 0, cvd = 0;
        // table mode: slot j holds id sid; its reported row, if any (rows ascend by id: the first
        // row with that id, the row k_prep's merge pointer reaches). Slot ids ascend strictly; a
        // slot repeating its predecessor's id is padding (pp_cartable.h pads with INT32_MAX, which
        // may also be a real car's id): it matches no row, as k_prep's merge pointer has already
        // passed that row. The group's lanes load the rows' ids (row p0 + q in lane q) and every
        // lane scans them by shuffles: one round trip to memory for the ids, not one per row
        // visited (the single-frame kernel waits for every one of those).
        int trow = -1, sid = 0;
        // (frames of at most G rows: the rows' cars come along with their ids, and the found row's
        // by a shuffle; the slot's stored state is read with its id: no load waits on the search)
        double fx = 0, fy = 0, fvx = 0, fvy = 0;
        bool fgot = false;
        int sv = 0, sln = 0;
        double ss = 0, sd = 0, svs = 0, svd = 0;
        if (tab) {
            const bool live = j < iters;
            const int64_t tix = (int64_t)j * S + s;
            sid = live ? (in.tab_id ? in.tab_id[tix] : j) : 0;
            if (live) {
                sv = in.tab_valid[tix]; sln = in.tab_lane[tix];
                ss = in.tab_s[tix]; sd = in.tab_d[tix]; svs = in.tab_vs[tix]; svd = in.tab_vd[tix];
            }
            bool done = !live || (in.tab_id && j > 0 && in.tab_id[tix - S] >= sid);
            for (int p0 = 0; p0 < ncar; p0 += G) {
                const int pl = p0 + r;
                int pid = 0;
                double px = 0, py = 0, pvx = 0, pvy = 0;
                if (p0 == 0) {                // (the rows loaded ahead)
                    if (pl < ncar) { pid = pid0; px = px0; py = py0; pvx = pvx0; pvy = pvy0; }
                } else if (pl < ncar) {
                    const int64_t ix = (int64_t)pl * S + s;
                    pid = in.car_id[ix];
                }
                const int nq = ncar - p0 < G ? ncar - p0 : G;
                for (int q = 0; q < nq; q++) {
                    const int cid = __shfl(pid, q, G);
                    if (!done && cid >= sid) { if (cid == sid) trow = p0 + q; done = true; }
                }
                if (ncar <= G) {              // (group-uniform)
                    const int src = trow >= 0 ? trow : 0;
                    fx = __shfl(px, src, G); fy = __shfl(py, src, G);
                    fvx = __shfl(pvx, src, G); fvy = __shfl(pvy, src, G);
                    fgot = trow >= 0;
                }
                if (grp_or<G>(done ? 0u : 1u) == 0u) break;
            }
        }
        PP_TRACE_K1(2);
        if (j < iters) {
            const int64_t tix = (int64_t)j * S + s;
            int row = j;
            if (tab) { row = trow; id = sid; }
            if (row >= 0) {
                const int64_t ix = (int64_t)row * S + s;
                double cx, cy, cvx, cvy;
                if (fgot) {                   // (tab: the row's id is the slot's)
                    cx = fx; cy = fy; cvx = fvx; cvy = fvy;
                } else if (!tab && j0 == 0) { // row j = r: loaded ahead
                    id = pid0;
                    cx = px0; cy = py0; cvx = pvx0; cvy = pvy0;
                } else {
                    id = in.car_id[ix];
                    cx = in.car_x[ix]; cy = in.car_y[ix]; cvx = in.car_vx[ix]; cvy = in.car_vy[ix];
                }
                if (draw > 0) car_noise(P, s, draw, row, cx, cy, cvx, cvy);
                int nwp = 0, clane = 0;
                if (lane_match(m, e.ref_wp, e.ratio, cx, cy, cs, cd, clane, nwp)) {
                    project_speed(m, cvx, cvy, nwp, cvs, cvd);
                    okl = 1 | (clane << 1);
                    if (tab) {
                        in.tab_valid[tix] = 1; in.tab_lane[tix] = clane;
                        in.tab_s[tix] = cs; in.tab_d[tix] = cd; in.tab_vs[tix] = cvs; in.tab_vd[tix] = cvd;
                        in.tab_vx[tix] = cvx; in.tab_vy[tix] = cvy;
                    }
                } else {
                    ust |= PP_ST_CAR_UNMATCHED;
                    if (tab) in.tab_valid[tix] = 0;
                }
            } else if (sv) {                  // (tab only) a stale slot
                okl = 1 | (sln << 1);
                cs = ss; cd = sd; cvs = svs; cvd = svd;
            }
        }
        PP_TRACE_K1(3);
        // the planner pass: the group's cars at once (PlanAcc::add_group), or one at a time
        if (grp_or<G>((okl & 1) && id == -1 ? 1u : 0u) == 0u) {
            a.add_group<G>(P, e, T_in, (okl & 1) != 0, j, id, cs, cd, okl >> 1, cvs, cvd);
        } else {
            const int nq = iters - j0 < G ? iters - j0 : G;
            for (int q = 0; q < nq; q++) {
                const int qokl = __shfl(okl, q, G);
                const int qid = __shfl(id, q, G);
                const double qcs = __shfl(cs, q, G), qcd = __shfl(cd, q, G);
                const double qcvs = __shfl(cvs, q, G), qcvd = __shfl(cvd, q, G);
                if (qokl & 1) a.add(P, e, T_in, j0 + q, qid, qcs, qcd, qokl >> 1, qcvs, qcvd);
            }
        }
    }
    PP_TRACE_K1(4);
    status |= grp_or<G>(ust);
    // prep_finish re-reads the follow cars' velocities from the slots other lanes of the group
    // (same wave) wrote above
    if (tab) __threadfence_block();
    prep_finish<G>(in, P, pv, info, out_status, gb, S, Sv, s, v, draw, tab, r, T_in, e, a, status);
    PP_TRACE_K1(5);
}

template <bool kLdsMap, int G>
__device__ __forceinline__ void prep_grp_body(MapG mg, pp_scene_batch in, pp_params P, PrepV pv,
                                              pp_scene_info* info, uint32_t* out_status, GroupBits gb) {
    static_assert(G >= 2 && G <= 16 && (G & (G - 1)) == 0, "group: a power of two in [2, 16]");
    extern __shared__ __attribute__((aligned(16))) double smap[];
    const int n = mg.n;
    if (kLdsMap) {
        stage_map(smap, mg.buf, kMapArrays * n);
        __syncthreads();
    }
    const MapV m = map_view(kLdsMap ? smap : mg.buf, n, mg.fastm);
    const int64_t Sv = in.n_scenes * (P.n_draws > 1 ? P.n_draws : 1);
    const int r = (int)(threadIdx.x % G);
    const int64_t v = (int64_t)blockIdx.x * (blockDim.x / G) + threadIdx.x / G;
    if (v >= Sv) return;                      // whole groups leave together
    prep_grp_eval<G>(m, in, P, pv, info, out_status, gb, v, r);
}

// the grouped instantiations by name (pp_eval's launch switch)
#define PP_PREP_GRP(NAME, G)                                                                         \
    template <bool kLdsMap>                                                                         \
    __global__ __launch_bounds__(256) void NAME(MapG mg, pp_scene_batch in, pp_params P, PrepV pv,  \
                                                pp_scene_info* info, uint32_t* os, GroupBits gb) {   \
        prep_grp_body<kLdsMap, G>(mg, in, P, pv, info, os, gb);                                     \
    }
PP_PREP_GRP(k_prep_g2, 2)
PP_PREP_GRP(k_prep_g4, 4)
PP_PREP_GRP(k_prep_g8, 8)
PP_PREP_GRP(k_prep_g16, 16)
#undef PP_PREP_GRP
