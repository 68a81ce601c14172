// pp_k_world.h — device: what surrounds the evaluator. The closed-loop rollout's simulator shim, judge
// and car-following, lane-changing traffic (k_sim, k_judge, k_follow, k_lane_change), the sensor model (k_sense), the tracker (k_track), the judge summary (k_summary_*), scene synthesis (k_synth*), the map tables'
// kernels (Map::Init, src/main.cpp:89-131) and k_libm. Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// closed-loop rollout: the simulator shim (include/pp.h pp_rollout). One lane per scene: log the
// frame, drive `consume` points of the plan, advance the traffic, report the cars in range.
// ------------------------------------------------------------------------------------------------
struct SimArgs {
    int consume;
    double range2;
    int frame;
    pp_rollout_log log;
};

__global__ __launch_bounds__(256) void k_sim(ppsynth::LaneTables LT, pp_scene_batch in,
                                             ppsynth::TrafficV tr, pp_params P, pp_result out, SimArgs A) {
    const int64_t S = in.n_scenes;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int N = P.n_points;
    const int n_out = out.n_out[s];
    const int T = out.winner[s] / P.n_speeds;
    double* ex = (double*)in.ego_x;
    double* ey = (double*)in.ego_y;
    double* eyaw = (double*)in.ego_yaw_deg;
    double* espd = (double*)in.ego_speed_mph;
    double* px = (double*)in.prev_x;
    double* py = (double*)in.prev_y;
    const double x0 = ex[s], y0 = ey[s];
    // frame record (the telemetry this frame was planned from + its plan)
    const int64_t fs = (int64_t)A.frame * S + s;
    if (A.log.ego_x) A.log.ego_x[fs] = x0;
    if (A.log.ego_y) A.log.ego_y[fs] = y0;
    if (A.log.ego_speed_mph) A.log.ego_speed_mph[fs] = espd[s];
    if (A.log.target_lane) A.log.target_lane[fs] = T;
    if (A.log.winner) A.log.winner[fs] = out.winner[s];
    if (A.log.n_out) A.log.n_out[fs] = n_out;
    if (A.log.status) A.log.status[fs] = out.status[s];
    if (A.log.n_cars) A.log.n_cars[fs] = in.n_cars[s];
    if (A.log.plan_x) {
        for (int i = 0; i < N; i++) {
            A.log.plan_x[((int64_t)A.frame * N + i) * S + s] = out.next_x[(int64_t)i * S + s];
            A.log.plan_y[((int64_t)A.frame * N + i) * S + s] = out.next_y[(int64_t)i * S + s];
        }
    }
    // ego: drive kk points; speed and yaw from the last driven step
    const int kk = n_out < A.consume ? n_out : A.consume;
    double nx = x0, ny = y0, qx = x0, qy = y0;
    if (kk >= 1) { nx = out.next_x[(int64_t)(kk - 1) * S + s]; ny = out.next_y[(int64_t)(kk - 1) * S + s]; }
    if (kk >= 2) { qx = out.next_x[(int64_t)(kk - 2) * S + s]; qy = out.next_y[(int64_t)(kk - 2) * S + s]; }
    const double dx = nx - qx, dy = ny - qy;
    const double dist = sqrt(dx * dx + dy * dy);
    ex[s] = nx; ey[s] = ny;
    espd[s] = dist * 50 * 2.237;
    if (dist > 0) eyaw[s] = ppg::atan2(dy, dx) * 180.0 / kPi;
    const int np = n_out - kk;
    for (int i = 0; i < PP_PREV_KEEP; i++) {
        const bool ok = i < np;
        px[(int64_t)i * S + s] = ok ? out.next_x[(int64_t)(kk + i) * S + s] : 0.0;
        py[(int64_t)i * S + s] = ok ? out.next_y[(int64_t)(kk + i) * S + s] : 0.0;
    }
    ((int32_t*)in.n_prev)[s] = np;
    ((int32_t*)in.prev_target_lane)[s] = T;
    // traffic: advance, then report the cars within range, ascending id
    int nc = 0;
    for (int j = 0; j < tr.n; j++) {
        const int64_t tx = (int64_t)j * S + s;
        const int lane = tr.lane[tx];
        int seg = tr.seg[tx];
        double t = tr.t[tx];
        const double v = tr.v[tx];
        ppsynth::lane_advance(LT, lane, &seg, &t, v * 0.02 * A.consume);
        tr.seg[tx] = seg; tr.t[tx] = t;
        double cx, cy, cvx, cvy;
        ppsynth::traffic_car(LT, lane, seg, t, tr.off[tx], v, &cx, &cy, &cvx, &cvy);
        const double rx = cx - nx, ry = cy - ny;
        if (rx * rx + ry * ry <= A.range2 && nc < in.car_stride) {
            const int64_t ix = (int64_t)nc * S + s;
            ((int32_t*)in.car_id)[ix] = j;
            ((double*)in.car_x)[ix] = cx; ((double*)in.car_y)[ix] = cy;
            ((double*)in.car_vx)[ix] = cvx; ((double*)in.car_vy)[ix] = cvy;
            nc++;
        }
    }
    ((int32_t*)in.n_cars)[s] = nc;
}

// The rollout judge (include/pp.h pp_judge_frame; csrc/pp_judge.h): one lane per scene, every array
// [k * S + s] so a wave's accesses are contiguous; no LDS, no scratch. Reads the pre-frame ego and
// traffic and the frame's plan, so it runs between pp_eval and k_sim; writes only the judge state.
__global__ __launch_bounds__(256) void k_judge(ppsynth::LaneTables LT, int64_t S, const double* ego_x,
                                               const double* ego_y, const double* ego_yaw_deg,
                                               const double* next_x, const double* next_y,
                                               const int32_t* n_out, ppsynth::TrafficV tr, int consume,
                                               pp_judge_cfg cfg, pp_judge st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    ppjudge::judge_scene(LT, S, s, ego_x[s], ego_y[s], ego_yaw_deg[s], next_x, next_y, n_out[s], tr, consume,
                         cfg, st);
}

// Reactive traffic (include/pp.h pp_traffic_follow; csrc/pp_follow.h): one lane per scene, every array
// [k * S + s]; no LDS, no scratch. Reads the pre-frame ego and traffic, so it runs before k_judge and
// k_sim; writes the traffic's speeds and the follow state.
__global__ __launch_bounds__(256) void k_follow(ppsynth::LaneTables LT, ppfollow::ArcTables AT, int64_t S,
                                                const double* ego_x, const double* ego_y,
                                                const double* ego_speed_mph, ppsynth::TrafficV tr, int consume,
                                                pp_follow_cfg cfg, pp_follow st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    ppfollow::follow_scene(LT, AT, S, s, ego_x[s], ego_y[s], ego_speed_mph[s], tr, consume, cfg, st);
}

// Lane-changing traffic (include/pp.h pp_traffic_lane_change; csrc/pp_lanechange.h): one lane per scene,
// every array [k * S + s]; no LDS, no scratch. Reads the pre-frame ego, the traffic with the speeds
// k_follow has just written and k_follow's records, so it runs after k_follow and before k_judge and
// k_sim; writes the traffic's lane, seg, t and offset and the lane-change state.
__global__ __launch_bounds__(256) void k_lane_change(ppsynth::LaneTables LT, ppfollow::ArcTables AT, int64_t S,
                                                     const double* ego_x, const double* ego_y,
                                                     const double* ego_speed_mph, ppsynth::TrafficV tr, int consume,
                                                     pp_follow_cfg fcfg, pp_follow fst, pp_lane_change_cfg cfg,
                                                     pp_lane_change st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    pplanechange::lane_change_scene(LT, AT, S, s, ego_x[s], ego_y[s], ego_speed_mph[s], tr, consume, fcfg, fst, cfg,
                                    st);
}

// The sensor model (include/pp.h pp_sense_frame; csrc/pp_sensor.h): one lane per scene, every array
// [r * S + s]; no LDS, no per-lane arrays. Reads the telemetry's ego position and car rows (the truth),
// so in a rollout it runs before pp_eval; writes only the sensor state. The occlusion loop reads the
// truth rows again from global memory (contiguous across the wave, served by L1/L2).
__global__ __launch_bounds__(256) void k_sense(ppsensor::Truth T, pp_sensor_cfg cfg, pp_sensor st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= T.S) return;
    ppsensor::sense_scene(T, s, cfg, st);
}

// The tracker (include/pp.h pp_track_frame; csrc/pp_tracker.h): one lane per scene, every array
// [. * S + s]; no LDS, no per-lane arrays: the merge walks two cursors, one into the rows and one into
// the old bank, through global memory. Reads the rows (the sensor state's or the telemetry's) and the
// old bank, writes the other bank and the tracked rows; in a rollout it runs between k_sense and pp_eval.
__global__ __launch_bounds__(256) void k_track(ppsensor::Truth Z, pp_tracker_cfg cfg, double dt, pp_tracker st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= Z.S) return;
    pptracker::track_scene(Z, s, cfg, dt, st);
}

// ------------------------------------------------------------------------------------------------
// Judge summary (include/pp.h pp_judge_summary; csrc/pp_summary.h): the world's one reduction across
// lanes and blocks. k_summary_tiles: one block of 256 per chunk of K consecutive 256-scene tiles of a
// group; in tile t lane i reads scene g E + 256 t + i of every array (contiguous), T_t is made per
// tile, everything else is kept per lane over the chunk and reduced once (block_part).
// k_summary_groups: one block per group, lane i the tiles t = i (mod 256) in ascending order and the
// chunks' parts. The FP64 sums are the fixed expression of pp_summary.h (no FP64 atomic anywhere);
// integers, minima and maxima are exact in any order, so no figure depends on K.
// ------------------------------------------------------------------------------------------------
struct SumArgs {
    int64_t S, E, G;              // scenes, scenes per group, groups
    int64_t tpg;                  // tiles of a full group
    int64_t cpg;                  // chunks of a full group, ceil(tpg / K) (the grid: G cpg blocks)
    int64_t R, out_first;         // rows the stats arrays hold, row of group 0
    double inv_w;                 // hist_bins / hist_max
    int B;                        // hist_bins
    int K;                        // tiles per chunk, 1..kSumChunkMax
    int direct;                   // tpg == 1: k_summary_tiles writes the rows itself, no records
};
constexpr int kSumChunkMax = 8;   // (block_part packs a wave's sums of the per-lane counts in 16 bits: 8 x 64 < 65,536)

// the workspace behind the chunks' parts: T_t of dist and of clean_dist per tile
struct SumRecs {
    ppsummary::Part* part;        // [g cpg + c]
    double* td;                   // [g tpg + t]
    double* tc;
};

template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) {        // every lane gets the wave's result
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v = op(v, __shfl_xor(v, w));
    return v;
}

// tree256 of the 256 values the block's lanes have stored in s_d and in s_c, after the barrier that
// follows the stores, by wave 0 (valid in its lane 0): w = 128 and 64 as one read of four LDS entries
// added in the tree's own order, w <= 32 as wave64 shuffles (lane i < w: v[i] += v[i + w]; what the
// lanes beyond compute is never read).
__device__ __forceinline__ void tree256_wave0(const double* s_d, const double* s_c, int lane, double& a, double& c) {
    a = (s_d[lane] + s_d[lane + 128]) + (s_d[lane + 64] + s_d[lane + 192]);
    c = (s_c[lane] + s_c[lane + 128]) + (s_c[lane + 64] + s_c[lane + 192]);
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        a = a + __shfl_down(a, w);
        c = c + __shfl_down(c, w);
    }
}

// The block's part from its 256 lanes' parts, all but the two sums, valid in thread 0 after the call
// (which holds one barrier): per wave by butterflies, the four waves' results combined through LDS.
// kPacked: the eight per-lane counts are a chunk's (at most kSumChunkMax) and go two to a 32-bit word.
template <bool kPacked>
__device__ __forceinline__ void block_part(ppsummary::Part& p, ppsummary::Part* s_w) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const auto add = [](long long a, long long b) { return a + b; };
    const auto uadd = [](uint32_t a, uint32_t b) { return a + b; };
    const auto umin = [](uint32_t a, uint32_t b) { return b < a ? b : a; };
    const auto dmin = [](double a, double b) { return b < a ? b : a; };
    const auto dmax = [](double a, double b) { return b > a ? b : a; };
    ppsummary::Part r;
    r.dist_sum = 0.0; r.clean_sum = 0.0; r.bin = -1;
    r.clean_min = wave_all(p.clean_min, dmin); r.clean_max = wave_all(p.clean_max, dmax);
    r.min_sep = wave_all(p.min_sep, dmin);
    r.max_mph = wave_all(p.max_mph, dmax); r.max_acc = wave_all(p.max_acc, dmax);
    r.max_jerk = wave_all(p.max_jerk, dmax);
    if (kPacked) {
        const uint32_t w0 = wave_all((uint32_t)p.n_unjudged | ((uint32_t)p.n_nonfinite << 16), uadd);
        const uint32_t w1 = wave_all((uint32_t)p.n_clean | ((uint32_t)p.with[0] << 16), uadd);
        const uint32_t w2 = wave_all((uint32_t)p.with[1] | ((uint32_t)p.with[2] << 16), uadd);
        const uint32_t w3 = wave_all((uint32_t)p.with[3] | ((uint32_t)p.with[4] << 16), uadd);
        static_assert(PP_INC_KINDS == 5, "the packing above holds five kinds");
        r.n_unjudged = w0 & 0xFFFF; r.n_nonfinite = w0 >> 16;
        r.n_clean = w1 & 0xFFFF; r.with[0] = w1 >> 16;
        r.with[1] = w2 & 0xFFFF; r.with[2] = w2 >> 16;
        r.with[3] = w3 & 0xFFFF; r.with[4] = w3 >> 16;
    } else {
        r.n_unjudged = wave_all((long long)p.n_unjudged, add);
        r.n_nonfinite = wave_all((long long)p.n_nonfinite, add);
        r.n_clean = wave_all((long long)p.n_clean, add);
#pragma unroll
        for (int k = 0; k < PP_INC_KINDS; k++) r.with[k] = wave_all((long long)p.with[k], add);
    }
    r.steps = wave_all((long long)p.steps, add);
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) {
        r.steps_in[k] = wave_all((long long)p.steps_in[k], add);
        r.first[k] = wave_all(p.first[k], umin);
    }
    if (lane == 0) s_w[wv] = r;
    __syncthreads();
    if (tid == 0) {
        p = s_w[0];
        ppsummary::merge(p, s_w[1]);
        ppsummary::merge(p, s_w[2]);
        ppsummary::merge(p, s_w[3]);
    }
}

// rows out_first .. out_first + G - 1 of the histogram to zero (k_summary_tiles adds into them)
__global__ __launch_bounds__(256) void k_summary_clear(SumArgs A, int64_t* hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.G * A.B) return;
    const int64_t b = i / A.G, g = i - b * A.G;
    hist[b * A.R + A.out_first + g] = 0;
}

// Chunk c of group g: tiles c K .. c K + K - 1 of the group, as far as it has scenes. Per tile: the
// lanes' parts, T_t of the two sums to td / tc [g tpg + t]; the other figures stay in the lane's
// running part and are reduced once per chunk into part [g cpg + c] (direct: into the row). The
// histogram: B 32-bit LDS counters per block, the non-zero ones flushed once per chunk by one 64-bit
// global integer add each. The sums' LDS arrays are double-buffered: a tile's stores go to the buffer
// wave 0 is not reading, and the next barrier is behind those reads.
__global__ __launch_bounds__(256) void k_summary_tiles(pp_judge st, SumArgs A, pp_judge_stats o, SumRecs rec) {
    __shared__ double s_d[2][ppsummary::kTile], s_c[2][ppsummary::kTile];
    __shared__ ppsummary::Part s_w[4];
    __shared__ uint32_t s_h[PP_STATS_MAX_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t g = blk / A.cpg, c = blk - g * A.cpg;
    const int64_t s0 = g * A.E, n = A.S - s0 < A.E ? A.S - s0 : A.E;
    const int64_t nt = ppsummary::n_tiles(n);
    const int64_t t0 = c * A.K, t1 = t0 + A.K < nt ? t0 + A.K : nt;
    for (int b = tid; b < A.B; b += 256) s_h[b] = 0;
    __syncthreads();
    ppsummary::Part acc;
    ppsummary::part_none(acc);
    double Td = 0.0, Tc = 0.0;
    for (int64_t t = t0; t < t1; t++) {                    // (uniform over the block)
        const int64_t k = t * ppsummary::kTile + tid;
        const int buf = (int)(t - t0) & 1;
        ppsummary::Part p;
        if (k < n) ppsummary::scene_part(st, A.S, s0 + k, A.inv_w, A.B, p); else ppsummary::part_none(p);
        if (p.bin >= 0) atomicAdd(&s_h[p.bin], 1u);
        s_d[buf][tid] = p.dist_sum;
        s_c[buf][tid] = p.clean_sum;
        ppsummary::merge(acc, p);
        __syncthreads();
        if (wv == 0) {
            tree256_wave0(s_d[buf], s_c[buf], lane, Td, Tc);
            if (lane == 0 && !A.direct) { rec.td[g * A.tpg + t] = Td; rec.tc[g * A.tpg + t] = Tc; }
        }
    }
    block_part<true>(acc, s_w);                            // (its barrier: the counters are complete)
    const int64_t row = A.out_first + g;
    for (int b = tid; b < A.B; b += 256) {
        const uint32_t h = s_h[b];
        if (h) atomicAdd((unsigned long long*)&o.hist[b * A.R + row], (unsigned long long)h);
    }
    if (tid != 0) return;
    if (A.direct) {                                        // one tile: u_0 = +0.0 + T_0, tree256(u) = u_0
        acc.dist_sum = 0.0 + Td;
        acc.clean_sum = 0.0 + Tc;
        ppsummary::write_row(o, A.R, row, n, acc);
    } else {
        rec.part[blk] = acc;
    }
}

__global__ __launch_bounds__(256) void k_summary_groups(SumArgs A, SumRecs rec, pp_judge_stats o) {
    __shared__ double s_d[ppsummary::kTile], s_c[ppsummary::kTile];
    __shared__ ppsummary::Part s_w[4];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t s0 = g * A.E, n = A.S - s0 < A.E ? A.S - s0 : A.E;
    const int64_t nt = ppsummary::n_tiles(n), nc = (nt + A.K - 1) / A.K;
    double ud = 0.0, uc = 0.0;
    for (int64_t t = tid; t < nt; t += ppsummary::kTile) {             // u_i from +0.0, ascending t
        ud = ud + rec.td[g * A.tpg + t];
        uc = uc + rec.tc[g * A.tpg + t];
    }
    s_d[tid] = ud;
    s_c[tid] = uc;
    ppsummary::Part p;
    ppsummary::part_none(p);
    for (int64_t c = tid; c < nc; c += ppsummary::kTile) ppsummary::merge(p, rec.part[g * A.cpg + c]);
    block_part<false>(p, s_w);                             // (its barrier: s_d and s_c are complete)
    if (tid >= 64) return;
    tree256_wave0(s_d, s_c, tid, ud, uc);
    if (tid != 0) return;
    p.dist_sum = ud;
    p.clean_sum = uc;
    ppsummary::write_row(o, A.R, A.out_first + g, n, p);
}

__global__ __launch_bounds__(256) void k_synth_traffic(ppsynth::LaneTables T, uint64_t seed, int64_t first,
                                                       ppsynth::OutBatch o, ppsynth::TrafficV tr, pp_scene_batch tb) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= o.S) return;
    ppsynth::synth_scene(T, seed, first + s, s, o, &tr);
    for (int j = 0; tb.tab_valid && j < tb.tab_slots; j++) {       // empty table, slot j = car j
        tb.tab_valid[(int64_t)j * o.S + s] = 0;
        if (tb.tab_id) tb.tab_id[(int64_t)j * o.S + s] = j;
    }
}

// Episode starts (include/pp.h pp_synth_episode; csrc/pp_episode.h): one lane per scene, every array
// [k * S + s]; no LDS but ppg::atan2's table, no scratch (the per-lane cursors are indexed only in
// unrolled select loops; the states come by value and go on by reference, never by address).
// Runs once per episode: telemetry, car table, traffic, and the judge and follow states when given.
__global__ __launch_bounds__(256) void k_synth_episode(ppsynth::LaneTables T, uint64_t seed, int64_t first,
                                                       pp_episode_cfg cfg, pp_follow_cfg gap, ppsynth::OutBatch o,
                                                       int32_t* tab_valid, int32_t* tab_id, int tab_slots,
                                                       ppsynth::TrafficV tr, pp_judge js, int has_js, pp_follow fs,
                                                       int has_fs) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= o.S) return;
    ppepisode::episode_scene(T, seed, first + s, s, cfg, gap, o, tab_valid, tab_id, tab_slots, tr,
                             js, has_js != 0, fs, has_fs != 0);
}

// ------------------------------------------------------------------------------------------------
// Map::Init on the device (src/main.cpp:89-131; pp_map_create_device). g: the MapG layout
// (kMapArrays n: ref x/y, normal x/y, lane centres x[NL]/y[NL], lane lengths[NL]); t: the synth
// lane tables (5 NL n). Three passes because each reads its neighbours' results of the previous one.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wrap_i(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

__global__ __launch_bounds__(256) void k_map_normals(const double* wx, const double* wy, int n, double* g,
                                                     int* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = wrap_i(i - 1, n);
    const double dx = wx[i] - wx[p], dy = wy[i] - wy[p];
    const double len = sqrt(dx * dx + dy * dy);
    if (!(len > 0)) atomicOr(bad, 1);                 // duplicate consecutive waypoints
    g[i] = wx[i]; g[n + i] = wy[i];
    g[2 * n + i] = dy / len;
    g[3 * n + i] = -dx / len;
}

__global__ __launch_bounds__(256) void k_map_lanes(int n, double* g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = wrap_i(i + 1, n);
    const double nx = g[2 * n + i], ny = g[3 * n + i];
    double ax = (nx + g[2 * n + q]) / 2, ay = (ny + g[3 * n + q]) / 2;
    // the host's std::atan2 / std::cos (glibc) restated bit for bit (pp_glibcm.h): the device map
    // equals pp_map_create's (|a_avg - a_n| < pi, inside the restated cos domain)
    const double a_n = ppg::atan2(ny, nx);
    const double a_avg = ppg::atan2(ay, ax);
    double c_;
    if (!ppg::cos(a_avg - a_n, c_)) c_ = __builtin_nan("");
    ax /= c_;
    ay /= c_;
    for (int r = 0; r < NL; r++) {
        const double off = 4.0 * (r + 0.5);
        g[(4 + r) * n + i] = g[i] + ax * off;
        g[(4 + NL + r) * n + i] = g[n + i] + ay * off;
    }
}

__global__ __launch_bounds__(256) void k_map_lengths(int n, double* g, double* t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = wrap_i(i - 1, n);
    for (int r = 0; r < NL; r++) {
        const double lx = g[(4 + r) * n + i], ly = g[(4 + NL + r) * n + i];
        const double dx = lx - g[(4 + r) * n + p], dy = ly - g[(4 + NL + r) * n + p];
        const double len = sqrt(dx * dx + dy * dy);
        g[(4 + 2 * NL + r) * n + i] = len;                           // Map::get_lane_length
        const double den = dx * dx + dy * dy;                         // helpers.h:202 rdenom
        g[(4 + 3 * NL + r) * n + i] = den;
        g[(4 + 4 * NL + r) * n + i] = 1.0 / den;
        t[0 * NL * n + r * n + i] = lx;
        t[1 * NL * n + r * n + i] = ly;
        t[2 * NL * n + r * n + i] = len;
        t[3 * NL * n + r * n + i] = dx / len;
        t[4 * NL * n + r * n + i] = dy / len;
    }
}

// the restated libm on the device (pp_libm_eval; parity tests of pp_glibcm.h's device build)
__global__ __launch_bounds__(256) void k_libm(int kind, const double* a, const double* b, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r = __builtin_nan("");
    if (kind == 0) ppg::sin(a[i], r);
    else if (kind == 1) ppg::cos(a[i], r);
    else r = ppg::atan2(a[i], b[i]);
    out[i] = r;
}

// ------------------------------------------------------------------------------------------------
// scene synthesis
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_synth(ppsynth::LaneTables T, uint64_t seed, int64_t first,
                                               ppsynth::OutBatch o) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= o.S) return;
    ppsynth::synth_scene(T, seed, first + s, s, o);
}
