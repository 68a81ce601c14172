// pp_diag.h — device: the diagnostic builds' hooks (-DPP_DIAG, -DPP_LIMCENSUS, -DPP_CENSUS, -DPP_CHECK,
// -DPP_TRACE): their device-side counters and the macros the kernels call, each one empty in the
// product build. Part of pp_eval.hip's translation unit.
#pragma once

#if defined(PP_DIAG) || defined(PP_LIMCENSUS)
// diagnostic builds only (-DPP_DIAG, -DPP_LIMCENSUS): per event, [2k] lanes where it fired,
// [2k+1] waves where any lane fired (the wave executes the branch). Read with pp_diag_read.
constexpr int kDiagWords = 96;
__device__ unsigned long long g_diag[kDiagWords];
__device__ __forceinline__ void diag(int k, bool c) {
    const unsigned long long b = __ballot(c);
    if (b && __lane_id() == (unsigned)__builtin_ctzll(__ballot(1))) {
        atomicAdd(&g_diag[2 * k], (unsigned long long)__builtin_popcountll(b));
        atomicAdd(&g_diag[2 * k + 1], 1ull);
    }
}
#endif
#ifdef PP_DIAG
#define PP_DIAGC(k, c) diag(k, c)
#else
#define PP_DIAGC(k, c) ((void)0)
#endif
// The limiter census (-DPP_LIMCENSUS; VERDICT r5 item 2, tests/test_full_batch.py): at every
// decision of the acceleration limiter (src/main.cpp:941 and :972) the census build also evaluates
// the reference's own operation sequence from the same state — the speed ramp's IEEE division,
// glibc's atan2 of the step (pp_glibcm.h, bit for bit) and the wrapped difference of absolute
// angles — and counts decisions within a relative 1e-12 of maximum_acc and decisions the two
// sequences take differently (g_diag events 26-33, names in tests/test_full_batch.py).
#ifdef PP_LIMCENSUS
#define PP_CEN(k, c) diag(k, c)
#else
#define PP_CEN(k, c) ((void)0)
#endif
#ifdef PP_CENSUS
// census builds only (-DPP_CENSUS): an assembly comment ";@R <output mode> <region>" at the start of
// each region of the candidate loop; tools/valu_census.py counts each region's instructions in the
// build's ISA and multiplies them by how often a wave executes the region (tools/diag_events.py)
#define PP_REGION(name) asm volatile(";@R %0 " name ::"i"(kOutMode))
#define PP_REGION_K(name) asm volatile(";@R 7 " name)
#define PP_REGION_A(name) asm volatile(";@R 8 " name)
#else
#define PP_REGION_A(name) ((void)0)
#define PP_REGION(name) ((void)0)
#define PP_REGION_K(name) ((void)0)
#endif
#ifdef PP_CHECK
// checking builds only (-DPP_CHECK): every global store of k_cand / k_emit (and the record reads
// of k_emit) is tested against the buffer it belongs to, and k_cand poisons its LDS slots at the
// start of every group, so a slot read that phase A of the same group did not write shows up as a
// NaN result or a meta sentinel. g_chk: [0] violations, [1] first site, [2] its offset, [3] its
// workgroup, [4] its group. Read with pp_check_read.
struct ChkLim {
    const double *paths, *nx, *ny, *rec, *cost;
    const unsigned long long* adjm;
    long long npaths, nnext, nrec, nadj, ncost, nscen;
};
__device__ unsigned long long g_chk[8];
__device__ ChkLim g_lim;
__device__ __forceinline__ bool chk_(bool ok, int site, long long off, long long grp) {
    if (!ok && atomicAdd(&g_chk[0], 1ull) == 0ull) {
        g_chk[1] = (unsigned long long)site; g_chk[2] = (unsigned long long)off;
        g_chk[3] = blockIdx.x; g_chk[4] = (unsigned long long)grp;
    }
    return ok;
}
// p inside [g_lim.B, g_lim.B + g_lim.N)
#define PP_CHKP(p, B, N, site) chk_((const void*)(p) >= (const void*)g_lim.B && (const void*)(p) < (const void*)(g_lim.B + g_lim.N), site, (long long)((const char*)(p) - (const char*)g_lim.B), -1)
#define PP_CHK(ok, site, off) chk_((ok), site, (long long)(off), -1)
constexpr int kMetaPoison = 0x7fffffff;
#else
#define PP_CHKP(p, B, N, site) true
#define PP_CHK(ok, site, off) true
#endif
#ifdef PP_TRACE
// diagnostic builds only (-DPP_TRACE): per workgroup of the traced kernel (k_cand<false>, and k_prep
// at kTraceK1 + blockIdx), 8 words: [0] start, [1] end of phase A, [2..5] end of phase B per wave,
// [6] end, [7] XCC id << 32 | HW_ID; times from the 100 MHz constant clock. Read with pp_trace_read.
constexpr int kTraceMax = 1 << 18, kTraceK1 = 3 << 16;
__device__ unsigned long long g_trace[8 * kTraceMax];
__device__ __forceinline__ void trace_at(unsigned long long blk, int k) {   // blk < kTraceMax
    g_trace[8 * blk + k] = wall_clock64();
}
__device__ __forceinline__ unsigned long long trace_hwid() {
    const unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));     // HW_REG_HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));    // HW_REG_XCC_ID
    return ((unsigned long long)xcc << 32) | hw;
}
#define PP_TRACE_AT(blk, k) do { if ((blk) < (unsigned)kTraceK1) trace_at((blk), (k)); } while (0)
// the grouped K1 of block 0 (k_step_small's single frame), lane 0: words at group kTraceK1 - 2
#define PP_TRACE_K1(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) trace_at(kTraceK1 - 2, (k)); } while (0)
#else
#define PP_TRACE_AT(blk, k) ((void)0)
#define PP_TRACE_K1(k) ((void)0)
#endif
