// pp_k_out.h — device: K3 and K4, the outputs. k_winner / k_winner_st (comfort mode: argmin, then the
// winner's re-run with outputs) and k_emit (reference mode: the replay of the recorded winner paths
// through the output transform, src/main.cpp:994-1007, 1033-1037).
// Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// K3: per-scene winner: argmin over the candidate costs (first minimum, as the oracle; with
// Monte-Carlo draws over the draw-averaged cost of each (lane, speed)), then the winning
// candidate re-run on the nominal scene with outputs.
// One lane per scene, 64 scenes per block; each lane's spline slot lives in LDS (kWinKnots =
// 9 previous + 6 control points, the real maximum) so 4 blocks fit a CU; with the segment cache
// the loop rarely reads it. next_x/next_y are point-major ([i * S + s], the batch's own
// convention): every step of the wave stores 512 contiguous bytes.
// ------------------------------------------------------------------------------------------------
// the winner's re-run with outputs (best: its candidate index; sl: its spline slot, built)
template <bool kSlow>
__device__ __forceinline__ void winner_run(const pp_scene_batch& in, const pp_params& P, const PrepV& pv,
                                           const pp_result& out, int64_t s, int64_t v0, int64_t Sv,
                                           int best, const Slot& sl) {
    const int64_t S = in.n_scenes;
    const int NS = P.n_speeds, N = P.n_points;
    const int L = best / NS, k = best - L * NS;
    const double v = cand_speed(P, pv.ego_speed[v0], k);
    const SC sc = make_sc(P, pv, Sv, v0, L, v);
    const int K = pv.K[v0];
    for (int i = 0; i < K; i++) {
        out.next_x[(int64_t)i * S + s] = in.prev_x[(int64_t)i * S + s];
        out.next_y[(int64_t)i * S + s] = in.prev_y[(int64_t)i * S + s];
    }
    const CandRes R = run_candidate<kSlow, 2>(P, sl, pv.pos_x[v0], pv.pos_y[v0], pv.angle[v0],
                                                    pv.ca_p[v0], pv.sa_p[v0], sc, N - K,
                                                    out.next_x + (int64_t)K * S + s,
                                                    out.next_y + (int64_t)K * S + s, S, nullptr, 0);
    for (int i = K + R.ng; i < N; i++) { out.next_x[(int64_t)i * S + s] = 0; out.next_y[(int64_t)i * S + s] = 0; }
    out.n_out[s] = K + R.ng;
    out.winner[s] = best;
}

template <bool kSlow>
__global__ __launch_bounds__(kWinBlock) void k_winner(MapG mg, pp_scene_batch in, pp_params P,
                                                      PrepV pv, pp_result out) {
    __shared__ __attribute__((aligned(16))) double wsm[5 * kWinKnots * kWinBlock];
    __shared__ int wmeta[4 * kWinBlock];
    const MapV m = map_view(mg.buf, mg.n);
    const int64_t S = in.n_scenes;
    const int D = P.n_draws > 1 ? P.n_draws : 1;
    const int64_t Sv = S * D;
    const int j = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * kWinBlock + j;
    const int64_t v0 = s * D;                 // the nominal (draw 0) prep record
    if (s >= S || ((pv.lim_mask[v0] & kLimSlow) != 0) != kSlow) return;
    const int NS = P.n_speeds, Cv = NL * NS, C = D * Cv;
    // decision: first minimum over (lane, k) of the cost averaged over the draws (summed in draw
    // order, then / D; D = 1: the plain cost)
    int best = 0;
    double bc = 0;
    for (int c = 0; c < Cv; c++) {
        double sum = out.cost[s * C + c];
        for (int d = 1; d < D; d++) sum += out.cost[s * C + d * Cv + c];
        const double mean = sum / D;
        if (out.draw_mean_cost) out.draw_mean_cost[s * Cv + c] = mean;
        if (c == 0 || mean < bc) { bc = mean; best = c; }
    }
    // slot arrays interleaved by lane ([knot][lane]) so the 64 lanes' accesses spread over banks
    const Slot sl = {wsm + j, wsm + kWinKnots * kWinBlock + j, wsm + 2 * kWinKnots * kWinBlock + j,
                     wsm + 3 * kWinKnots * kWinBlock + j, wsm + 4 * kWinKnots * kWinBlock + j,
                     wmeta + j, kWinBlock, kWinBlock};
    setup_lane(m, P, in, pv, s, v0, Sv, best / NS, sl);
    winner_run<kSlow>(in, P, pv, out, s, v0, Sv, best, sl);
}

// Round 6: k_cand made the decision (out.winner) and stored the winner's spline slot (per scene
// kWinRec doubles: the knot-interleaved x, y, a, b, c of k_cand's LDS slot, then the 4 meta ints):
// no argmin, no spline build and no LDS here, so the block is 256 lanes and occupancy is the
// registers' (k_winner holds 38 KB of LDS per 64 lanes: one wave per SIMD). A segment reload reads
// one knot's 40 contiguous bytes, and the cache line holding them usually holds the next knot too.
template <bool kSlow>
__global__ __launch_bounds__(256) void k_winner_st(pp_scene_batch in, pp_params P, PrepV pv, pp_result out,
                                                   const double* wslot) {
    const int64_t S = in.n_scenes;
    const int D = P.n_draws > 1 ? P.n_draws : 1;
    const int64_t Sv = S * D;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v0 = s * D;
    if (s >= S || ((pv.lim_mask[v0] & kLimSlow) != 0) != kSlow) return;
    double* b = const_cast<double*>(wslot) + s * kWinRec;
    const Slot sl = {b, b + 1, b + 2, b + 3, b + 4, (int*)(b + 5 * kWinKnots), 5, 1};
    winner_run<kSlow>(in, P, pv, out, s, v0, Sv, out.winner[s], sl);
}


// ------------------------------------------------------------------------------------------------
// K4 (reference mode): next_x/next_y of the winner from its recorded local path — the output
// transform of TrajectoryBuilder::build replayed exactly: at each recorded curvature adjustment
// the transform centre is rotated about the current point and the frame angle advanced
// (src/main.cpp:994-1007), every point is mapped back with the current frame (:1033-1037). One lane
// per scene; all loads/stores point-major (coalesced).
// ------------------------------------------------------------------------------------------------
// kChunk: recorded steps loaded together per lane (kEmitChunk for large batches; small batches,
// where the kernel is one serial chain of memory round trips per lane, load 16 steps at a time)
template <int kChunk>
__device__ __forceinline__ void emit_scene(const pp_scene_batch& in, const pp_params& P, const PrepV& pv,
                                           const pp_result& out, const double* rec, const uint64_t* adjm,
                                           int64_t s) {
    const int64_t S = in.n_scenes;
    const int N = P.n_points;
    const int K = pv.K[s];
    const int room = N - K;
    const int ng = out.n_out[s] - K;
    const int64_t rstride = (int64_t)room * S;
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
    const uint64_t m0 = adjm[s], m1 = adjm[S + s];
    double pxp = 0, pyp = 0;                       // local position before the step
    // The adjusted steps are sparse and scattered over the wave's lanes, so the turn block runs,
    // with few lanes active, on most steps: it is kept short (frame_turn, turn_sincos). Steps are
    // taken kChunk at a time with all of the chunk's record loads (the turn angle only where the
    // step's bit is set) in flight together: one memory round trip per chunk instead of one or two
    // per step. A turn beyond sincos_pp's medium range (a step that slowed to ~1e-7 m/s) sends the
    // lane's chunk through a per-step loop with the library reduction, re-reading the record: the
    // unrolled chunk then holds no call and stays register-light.
    for (int g0 = 0; g0 < ng; g0 += kChunk) {
        double px_[kChunk], py_[kChunk], rt[kChunk];
        uint32_t bits = 0;
#pragma unroll
        for (int u = 0; u < kChunk; u++) {
            const int g = g0 + u;
            const bool bit = g < ng && ((g < 64 ? (m0 >> g) & 1 : (m1 >> (g - 64)) & 1) != 0);
            bits |= bit ? 1u << u : 0u;
#ifdef PP_CHECK
            if (g < ng) { PP_CHKP(rec_py((double*)rec, rstride, g, S, s), rec, nrec, 16); }
            if (bit) { PP_CHKP(rec_rot(rec, rstride, g, S, s), rec, nrec, 16); }
#endif
            px_[u] = 0.0; py_[u] = 0.0;
            if (g < ng) rec_ld(rec, rstride, g, S, s, px_[u], py_[u]);
            rt[u] = bit ? PP_LD(rec_rot(rec, rstride, g, S, s)) : 0.0;
        }
        bool huge = false;
#pragma unroll
        for (int u = 0; u < kChunk; u++) huge |= !(fabs(rt[u]) <= ppm::kMediumMax);
        if (__builtin_expect(huge, 0)) {
            for (int g = g0; g < ng && g < g0 + kChunk; g++) {
                if ((g < 64 ? (m0 >> g) & 1 : (m1 >> (g - 64)) & 1) != 0) {
                    double cr, sr;
                    turn_sincos<true>(*rec_rot(rec, rstride, g, S, s), sr, cr);
                    frame_turn(F, pxp, pyp, cr, sr);
                }
                double qx, qy, ox, oy;
                rec_ld(rec, rstride, g, S, s, qx, qy);
                frame_pt(F, qx, qy, ox, oy);
                out.next_x[(int64_t)(K + g) * S + s] = ox;
                out.next_y[(int64_t)(K + g) * S + s] = oy;
                pxp = qx;
                pyp = qy;
            }
            continue;
        }
        // sin/cos of the chunk's turns first (rt = 0 where no turn): independent of each other and
        // of the chain of turns below, so they overlap instead of queueing behind it
        double crs[kChunk], srs[kChunk];
        if (bits) {
#pragma unroll
            for (int u = 0; u < kChunk; u++) turn_sincos<false>(rt[u], srs[u], crs[u]);
        }
        // (not unrolled: the exits keep the compiler from it, as in emit_scene_rows below)
        for (int u = 0; u < kChunk; u++) {
            const int g = g0 + u;
            if (g >= ng) break;
            if ((bits >> u) & 1) frame_turn(F, pxp, pyp, crs[u], srs[u]);
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

// k_emit by output rows: the lane's loop runs over next_x/next_y's rows i = 0 .. N-1 (kept previous
// point i < K, generated point g = i - K < ng, zero after), so every store of the wave goes to one
// row (512 contiguous bytes), where stepping by g scatters each store over the rows K + g of the
// wave's lanes (K = 0 ... 9) and leaves every written line partial. The record loads are the ones
// scattered instead (rows g = i - K), read through the cache, where the wave's other lanes of the
// same line find them. Same operations in the same order per lane as emit_scene: bit-identical.
template <int kChunk>
__device__ __forceinline__ void emit_scene_rows(const pp_scene_batch& in, const pp_params& P, const PrepV& pv,
                                                const pp_result& out, const double* rec, const uint64_t* adjm,
                                                int64_t s) {
    const int64_t S = in.n_scenes;
    const int N = P.n_points;
    const int K = pv.K[s];
    const int room = N - K;
    const int ng = out.n_out[s] - K;
    const int64_t rstride = (int64_t)room * S;
    OutFrame F = {pv.pos_x[s], pv.pos_y[s], pv.ca_p[s], pv.sa_p[s]};
    const uint64_t m0 = adjm[s], m1 = adjm[S + s];
    double pxp = 0, pyp = 0;                       // local position before the step
    for (int i0 = 0; i0 < N; i0 += kChunk) {
        double px_[kChunk], py_[kChunk], rt[kChunk];
        uint32_t bits = 0, gen = 0;
#pragma unroll
        for (int u = 0; u < kChunk; u++) {
            const int i = i0 + u, g = i - K;
            const bool isg = i < N && g >= 0 && g < ng;
            const bool bit = isg && ((g < 64 ? (m0 >> g) & 1 : (m1 >> (g - 64)) & 1) != 0);
            bits |= bit ? 1u << u : 0u;
            gen |= isg ? 1u << u : 0u;
#ifdef PP_CHECK
            if (isg) { PP_CHKP(rec_py((double*)rec, rstride, g, S, s), rec, nrec, 16); }
            if (bit) { PP_CHKP(rec_rot(rec, rstride, g, S, s), rec, nrec, 16); }
#endif
            px_[u] = 0.0; py_[u] = 0.0;
            if (isg) {
                px_[u] = *rec_px((double*)rec, rstride, g, S, s);
                py_[u] = *rec_py((double*)rec, rstride, g, S, s);
            } else if (i < K) {
                px_[u] = in.prev_x[(int64_t)i * S + s];
                py_[u] = in.prev_y[(int64_t)i * S + s];
            }
            rt[u] = bit ? *rec_rot(rec, rstride, g, S, s) : 0.0;
        }
        bool huge = false;
#pragma unroll
        for (int u = 0; u < kChunk; u++) huge |= !(fabs(rt[u]) <= ppm::kMediumMax);
        if (__builtin_expect(huge, 0)) {
            // a turn beyond the medium range: the chunk step by step with the library reduction,
            // re-reading its inputs (the unrolled path below then holds no call)
            for (int i = i0; i < N && i < i0 + kChunk; i++) {
                const int g = i - K;
                double ox = 0.0, oy = 0.0;
                if (g >= 0 && g < ng) {
                    if ((g < 64 ? (m0 >> g) & 1 : (m1 >> (g - 64)) & 1) != 0) {
                        double cr, sr;
                        turn_sincos<true>(*rec_rot(rec, rstride, g, S, s), sr, cr);
                        frame_turn(F, pxp, pyp, cr, sr);
                    }
                    const double qx = *rec_px((double*)rec, rstride, g, S, s);
                    const double qy = *rec_py((double*)rec, rstride, g, S, s);
                    frame_pt(F, qx, qy, ox, oy);
                    pxp = qx;
                    pyp = qy;
                } else if (i < K) {
                    ox = in.prev_x[(int64_t)i * S + s];
                    oy = in.prev_y[(int64_t)i * S + s];
                }
                out.next_x[(int64_t)i * S + s] = ox;
                out.next_y[(int64_t)i * S + s] = oy;
            }
            continue;
        }
        double crs[kChunk], srs[kChunk];
        if (bits) {
#pragma unroll
            for (int u = 0; u < kChunk; u++) turn_sincos<false>(rt[u], srs[u], crs[u]);
        }
        // (a loop, not unrolled: its two exits keep the compiler from unrolling it, and the
        // unrolled form, written with guards instead of exits, measured 4 % slower: k_emit 0.79 ->
        // 0.82 ms at config 5, profiles/r04_ablations.txt)
        for (int u = 0; u < kChunk; u++) {
            const int i = i0 + u;
            if (i >= N) break;
            double ox = px_[u], oy = py_[u];
            if ((gen >> u) & 1) {
                if ((bits >> u) & 1) frame_turn(F, pxp, pyp, crs[u], srs[u]);
                frame_pt(F, px_[u], py_[u], ox, oy);
                pxp = px_[u];
                pyp = py_[u];
            }
            if (!PP_CHKP(out.next_x + (int64_t)i * S + s, nx, nnext, 17)) break;
            PP_ST(out.next_x + (int64_t)i * S + s, ox);
            PP_ST(out.next_y + (int64_t)i * S + s, oy);
        }
    }
}

// 4 waves per SIMD (128 VGPRs): the 262,144-scene shard's k_emit 0.108 -> 0.098 ms, the full
// config-5 batch unchanged (profiles/r03_ablations.txt)
constexpr int kEmitWaves = 4;
template <int kChunk>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kEmitWaves))) void k_emit(pp_scene_batch in, pp_params P, PrepV pv, pp_result out,
                                              const double* rec, const uint64_t* adjm, int64_t s0, int64_t s1) {
    const int64_t s = s0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // scenes [s0, s1)
    if (s >= s1 || s >= in.n_scenes) return;
    if (kChunk == kEmitRows) emit_scene_rows<kChunk>(in, P, pv, out, rec, adjm, s);
    else emit_scene<kChunk>(in, P, pv, out, rec, adjm, s);
}
