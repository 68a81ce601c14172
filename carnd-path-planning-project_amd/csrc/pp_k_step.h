// pp_k_step.h — device: the fused launches of small reference-mode batches and of the single frame:
// k_cand_small (K2 + K4), k_step_small / k_step_small512 (K1 + K2 + K4) and k_plan_frame (the same
// step with the frame's input and output copies). They restate no reference code of their own: every
// stage is the function its own kernel calls. Part of pp_eval.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------------------------
// K2 + K4 in one launch for small batches in reference mode (no paths), where the step is a chain
// of kernel latencies (BASELINE config 2: 4,096 scenes, ~1 wave per SIMD): the group's scenes in
// the proven range (k_cand<false>'s code), then its flagged scenes (k_cand<true>'s code; the
// group's bitmap bit is cleared as k_cand<true> clears it), then the lanes that recorded the
// winners' paths (tid < nsc, kMode 1) replay the output transform from their own stores
// (emit_scene). Two kernel boundaries fewer; waves_per_eu(1, 2): registers are not the limit here.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_cand_small(
        MapG mg, pp_scene_batch in, pp_params P, PrepV pv, pp_result out, int SPB, double* rec,
        uint64_t* adjm, uint32_t* gbits) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t g = blockIdx.x;
    cand_group<false, 1, 1>(mg, in, P, pv, out, SPB, 1, rec, adjm, g, sm);
    __syncthreads();
    if ((gbits[g >> 5] >> (g & 31)) & 1u) {                   // same word for every lane
        cand_group<true, 1, 1>(mg, in, P, pv, out, SPB, 1, rec, adjm, g, sm);
        if (threadIdx.x == 0) atomicAnd(&gbits[g >> 5], ~(1u << (g & 31)));
    }
}

// ------------------------------------------------------------------------------------------------
// The whole step in one launch for small batches in reference mode (BASELINE config 2): K1 for the
// block's SPB (<= 16) scenes with 16 lanes each (prep_grp_eval<16>, the map staged in LDS once),
// a barrier, then k_cand_small's body (fast scenes, flagged scenes, the winners' replay), its
// phase A reading the same LDS map. The prep record goes through global memory inside the block
// (written, barrier, read by the same workgroup). No kernel boundary is left in the step.
// ------------------------------------------------------------------------------------------------
// the winners' output in the one-launch step (cand_group kEmitIn): inline (2) or replayed (1)
constexpr int kStepEmit = 2;
__device__ __forceinline__ void step_small_body(MapG mg, const pp_scene_batch& in, const pp_params& P,
                                                const PrepV& pv, const pp_result& out, int SPB, double* rec,
                                                uint64_t* adjm) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = mg.n;
#ifdef PP_TRACE
    // (block 0: start, after K1, after the fast scenes' K2 + K4, end; words at group kTraceK1 - 1;
    // the shader clock (s_memtime) beside the constant clock at start and end, group kTraceK1 - 3)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        trace_at(kTraceK1 - 1, 0);
        g_trace[8 * (kTraceK1 - 3) + 0] = wall_clock64();
        g_trace[8 * (kTraceK1 - 3) + 1] = clock64();
    }
#endif
    stage_map(sm, mg.buf, kMapArrays * n);
    __syncthreads();
    const MapV m = map_view(sm, n, mg.fastm);
    const int64_t g = blockIdx.x;
    {   // K1: scene g SPB + threadIdx.x / 16 by a group of 16 lanes
        const int q = (int)threadIdx.x / 16;
        const int64_t v = g * SPB + q;
        const GroupBits nobits = {nullptr, SPB, 1, nullptr, nullptr};
        if (q < SPB && v < in.n_scenes) prep_grp_eval<16>(m, in, P, pv, out.info, out.status, nobits, v, (int)threadIdx.x % 16);
    }
    __syncthreads();
#ifdef PP_TRACE
    if (blockIdx.x == 0 && threadIdx.x == 0) trace_at(kTraceK1 - 1, 1);
#endif
    const MapG ml = {sm, n, mg.fastm};
    double* csm = sm + ((kMapArrays * n + 1) & ~1);
    cand_group<false, 1, kStepEmit>(ml, in, P, pv, out, SPB, 1, rec, adjm, g, csm);
    __syncthreads();
#ifdef PP_TRACE
    if (blockIdx.x == 0 && threadIdx.x == 0) trace_at(kTraceK1 - 1, 2);
#endif
    cand_group<true, 1, kStepEmit>(ml, in, P, pv, out, SPB, 1, rec, adjm, g, csm);
#ifdef PP_TRACE
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        trace_at(kTraceK1 - 1, 3);
        g_trace[8 * (kTraceK1 - 3) + 2] = wall_clock64();
        g_trace[8 * (kTraceK1 - 3) + 3] = clock64();
    }
#endif
}
// The one-launch step with phase A off the critical path (k_plan_frame, and k_step_small for blocks
// of up to kStepWaveSpb scenes): waves 0-1 run K1 (16 lanes per scene) while waves 2-3 derive each
// scene's ego state and the build's start pose themselves (K1's own functions on the same inputs:
// the same bits as K1's record) and build the scenes' NL spline slots — phase A needs neither the
// cars nor the planner. Wave 2 takes scenes 0-3, wave 3 scenes 4-7; each wave's steps synchronise
// by wave (one instruction stream; LDS is in order within a wave), the per-scene geometry passing
// through an LDS record of kGeoD doubles per scene.
constexpr int kStepWaveSpb = 8;
constexpr int kGeoD = 17;           // (the last: the heading)
static_assert(9 + NL <= kGeoD - 1, "geometry record");
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// wave w of the phase-A waves, lane l: scenes [4 w, 4 w + 4) of the block's nsc
__device__ __forceinline__ void wave_phase_a(const MapV& m, const pp_scene_batch& in, const pp_params& P,
                                             const PrepV& pv, int SPB, double* sm, double* geo, int64_t s0,
                                             int nsc, int w, int l) {
    const int64_t S = in.n_scenes;
    {   // the ego state, start pose and rotations of scene q by 16 lanes; lane 0 records them
        const int q = 4 * w + l / 16, r = l % 16;
        if (q < nsc) {                                // (group-uniform)
            const int64_t s = s0 + q;
            EgoSt e;
            prep_ego<16>(m, in, P, S, s, r, e);
            double pos_x, pos_y, angle;
            start_pose(in, S, s, e, pos_x, pos_y, angle);
            double tv[4];
            frame_trig<16>(angle, r, tv);
            const double ca_m = __shfl(tv[0], 0, 16), sa_m = __shfl(tv[1], 1, 16);
            // the prep record's pose and rotations (K1 skips them: GroupBits.pose_by_wave)
            double* const tdst[4] = {pv.ca_m, pv.sa_m, pv.ca_p, pv.sa_p};
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (t == r) tdst[t][s] = tv[t];
            if (r == 0) { pv.pos_x[s] = pos_x; pv.pos_y[s] = pos_y; pv.angle[s] = angle; }
            if (r == 0) {
                double* gq = geo + q * kGeoD;
                gq[kGeoD - 1] = angle;
                gq[0] = e.K; gq[1] = pos_x; gq[2] = pos_y; gq[3] = ca_m; gq[4] = sa_m; gq[5] = e.ref_wp;
                gq[6] = e.ego_d; gq[7] = e.ego_speed; gq[8] = e.ego_vd;
#pragma unroll
                for (int k = 0; k < NL; k++) gq[9 + k] = e.ratio[k];
            }
        }
    }
    wave_sync();
    const int nslot = NL * SPB;
    double* sX = sm;
    int* sMeta = (int*)(sX + 5 * nslot * kKP);
    constexpr int kTS = 64 / (4 * NL) < 8 ? 64 / (4 * NL) : 8;
    const int jj = l / kTS, r = l - jj * kTS;         // this wave's slot jj (scene 4 w + jj / NL)
    const int q = 4 * w + jj / NL, L = jj % NL;
    const bool act = jj < 4 * NL && q < nsc;
    const int js = l, qs = 4 * w + js / NL;           // the serial steps: one lane per slot
    const bool act_s = js < 4 * NL && qs < nsc;
    auto geom = [&](int qq, int LL) {
        const double* gq = geo + qq * kGeoD;
        double ratio_L = gq[9];
#pragma unroll
        for (int k = 1; k < NL; k++) if (LL == k) ratio_L = gq[9 + k];
        return lane_geom_from((int)gq[0], gq[1], gq[2], gq[3], gq[4], (int)gq[5], ratio_L, gq[6], gq[7], gq[8], LL);
    };
    const Slot sl = lds_slot(sX, nslot, sMeta, act ? q * NL + L : 0);
    const Slot sls = lds_slot(sX, nslot, sMeta, act_s ? qs * NL + js % NL : 0);
    if (act) team_a1(m, in, geom(q, L), s0 + q, L, sl, r, kTS);
    wave_sync();
    if (act_s) team_a2(geom(qs, js % NL), sls);
    wave_sync();
    if (act) team_a3(sl, r, kTS);
    wave_sync();
    if (act_s) team_a4(sls);
    wave_sync();
    if (act) team_a5(sl, r, kTS);
}

// block g: scenes [g SPB, g SPB + nsc), SPB <= kThreads / 32: the first half of the block runs K1
// (16 lanes per scene), the second half phase A (4 scenes per wave)
template <int kThreads>
__device__ __forceinline__ void wave_step_body(MapG mg, const pp_scene_batch& in, const pp_params& P,
                                               const PrepV& pv, const pp_result& out, int SPB, double* rec,
                                               uint64_t* adjm, double* geo) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = mg.n;
    const int64_t g = blockIdx.x, s0 = g * SPB;
    const int nsc = (int)(in.n_scenes - s0 < SPB ? in.n_scenes - s0 : SPB);
#ifdef PP_TRACE
    if (blockIdx.x == 0 && threadIdx.x == 0) trace_at(kTraceK1 - 1, 0);
#endif
    stage_map(sm, mg.buf, kMapArrays * n);
    __syncthreads();
    const MapV m = map_view(sm, n, mg.fastm);
    double* csm = sm + ((kMapArrays * n + 1) & ~1);
    const int tid = (int)threadIdx.x;
    if (tid < kThreads / 2) {                     // K1: scene s0 + tid / 16 by 16 lanes
        const int q = tid / 16;
        const GroupBits nobits = {nullptr, SPB, 1, nullptr, nullptr, 1};
        if (q < nsc) prep_grp_eval<16>(m, in, P, pv, out.info, out.status, nobits, s0 + q, tid % 16);
    } else {
        wave_phase_a(m, in, P, pv, SPB, csm, geo, s0, nsc, (tid - kThreads / 2) / 64, tid % 64);
#ifdef PP_TRACE
        if (blockIdx.x == 0 && tid == kThreads / 2) trace_at(kTraceK1 - 4, 0);
#endif
    }
    __syncthreads();
    // the heading's kLimSlow bit (recorded by the phase-A waves), before cand_group's first read
    // of lim_mask (behind its first barrier)
    if (tid < nsc && !(fabs(geo[tid * kGeoD + kGeoD - 1]) <= kSlowAngle))
        pv.lim_mask[s0 + tid] |= kLimSlow;
#ifdef PP_TRACE
    if (blockIdx.x == 0 && tid == 0) trace_at(kTraceK1 - 1, 1);
#endif
    const MapG ml = {sm, n, mg.fastm};
    cand_group<false, 1, kStepEmit, true>(ml, in, P, pv, out, SPB, 1, rec, adjm, g, csm);
    __syncthreads();
#ifdef PP_TRACE
    if (blockIdx.x == 0 && tid == 0) trace_at(kTraceK1 - 1, 2);
#endif
    cand_group<true, 1, kStepEmit>(ml, in, P, pv, out, SPB, 1, rec, adjm, g, csm);
#ifdef PP_TRACE
    if (blockIdx.x == 0 && tid == 0) trace_at(kTraceK1 - 1, 3);
#endif
}

// waves (host: step_waves_on): the block runs wave_step_body (SPB <= kStepWaveSpb, 256 threads, the
// geometry records in LDS after k_cand's)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_step_small(
        MapG mg, pp_scene_batch in, pp_params P, PrepV pv, pp_result out, int SPB, double* rec,
        uint64_t* adjm, int waves) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if (waves) {                                  // (launch-uniform)
        double* geo = sm + ((kMapArrays * mg.n + 1) & ~1) + CandLds{SPB}.doubles();
        wave_step_body<256>(mg, in, P, pv, out, SPB, rec, adjm, geo);
    } else {
        step_small_body(mg, in, P, pv, out, SPB, rec, adjm);
    }
}

// 512 threads: blocks of 16 scenes, K1 on waves 0-3 beside phase A on waves 4-7 (BASELINE config 2:
// 256 such blocks, one per CU)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_step_small512(
        MapG mg, pp_scene_batch in, pp_params P, PrepV pv, pp_result out, int SPB, double* rec,
        uint64_t* adjm) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* geo = sm + ((kMapArrays * mg.n + 1) & ~1) + CandLds{SPB}.doubles();
    wave_step_body<512>(mg, in, P, pv, out, SPB, rec, adjm, geo);
}

// ------------------------------------------------------------------------------------------------
// pp_plan_frame in one launch: the frame's input ranges are read from pinned host memory into the
// device frame by the block itself, k_step_small's body runs, the output ranges are written back
// to pinned host memory, and a sequence number in host memory tells the waiting host thread the
// frame is done — no copy commands and no stream synchronisation per frame.
// Ranges are 16-byte-unit ranges of the frame (host and device share the layout; the host rounds
// each field's range out to whole units and merges neighbours): one 16-B load per unit, since
// the reads cross PCIe as one transaction per load.
// ------------------------------------------------------------------------------------------------
constexpr int kFioMax = 16;
constexpr int kFioInline = 176;   // 16-B units of input carried in the kernel arguments (2.75 KB)
struct FrameIO {
    const uint4* h_in;        // pinned host frame (inputs)
    uint4* d_frame;           // device frame
    uint4* h_out;             // pinned host frame (outputs)
    uint32_t* h_flag;         // pinned host word: seq once the outputs are in place
    uint32_t seq;
    int n_in, n_out;
    uint32_t in_off[kFioMax], in_len[kFioMax], out_off[kFioMax], out_len[kFioMax];   // 16-B units
    // inputs of up to kFioInline units (a frame of up to ~25 cars) ride in the kernel arguments,
    // which the launch writes to device memory: the block reads them there instead of across
    // PCIe (n_inl: the units held, in range order; 0: read the ranges from h_in)
    int n_inl;
    uint4 inl[kFioInline];
};
// units [0, total) of the ranges, thread t taking t, t + blockDim.x, ...: every thread's loads are
// issued before its stores (one round trip to the host per kChunk units)
template <int kChunk>
__device__ __forceinline__ void frame_copy(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                           int nr, const uint32_t* off, const uint32_t* len) {
    uint32_t total = 0;
    for (int r = 0; r < nr; r++) total += len[r];
    for (uint32_t w0 = threadIdx.x; w0 < total; w0 += kChunk * blockDim.x) {
        uint4 v[kChunk];
        uint32_t at[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; u++) {
            uint32_t w = w0 + u * blockDim.x;
            at[u] = 0xffffffffu;
            if (w < total) {
                int r = 0;
                while (w >= len[r]) { w -= len[r]; r++; }
                at[u] = off[r] + w;
                v[u] = src[at[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < kChunk; u++)
            if (at[u] != 0xffffffffu) dst[at[u]] = v[u];
    }
}
// (io is the first kernel argument: offset 0 of the kernel-argument segment)
constexpr size_t kFioArgOff = 0;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_plan_frame(
        FrameIO io, MapG mg, pp_scene_batch in, pp_params P, PrepV pv, pp_result out, int SPB, double* rec,
        uint64_t* adjm, int waves) {
#ifdef PP_FRAME_PROF
    const uint64_t t_in = wall_clock64();
#endif
    if (io.n_inl > 0) {
        // the kernel-argument copy: units in range order (thread t: units t, t + blockDim.x)
        const uint4* src = (const uint4*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + kFioArgOff +
                                          offsetof(FrameIO, inl));
        for (int w0 = (int)threadIdx.x; w0 < io.n_inl; w0 += (int)blockDim.x) {
            int w = w0, r = 0;
            while (w >= (int)io.in_len[r]) { w -= (int)io.in_len[r]; r++; }
            io.d_frame[io.in_off[r] + w] = src[w0];
        }
    } else {
        frame_copy<4>(io.h_in, io.d_frame, io.n_in, io.in_off, io.in_len);
    }
    __threadfence_block();
    __syncthreads();
#ifdef PP_FRAME_PROF
    const uint64_t t_body = wall_clock64();
#endif
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if (waves) {
        double* geo = sm + ((kMapArrays * mg.n + 1) & ~1) + CandLds{SPB}.doubles();
        wave_step_body<256>(mg, in, P, pv, out, SPB, rec, adjm, geo);
    } else {
        step_small_body(mg, in, P, pv, out, SPB, rec, adjm);
    }
    __threadfence_block();
    __syncthreads();
#ifdef PP_FRAME_PROF
    const uint64_t t_out = wall_clock64();
#endif
    frame_copy<4>(io.d_frame, io.h_out, io.n_out, io.out_off, io.out_len);
#ifdef PP_FRAME_PROF
    if (threadIdx.x == 0) { io.h_flag[4] = (uint32_t)t_in; io.h_flag[5] = (uint32_t)t_body; io.h_flag[6] = (uint32_t)t_out; io.h_flag[7] = (uint32_t)wall_clock64(); }
#endif
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(io.h_flag, io.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
