// pp_summary.h — the grouped summary of a judge state (include/pp.h pp_judge_summary; DESIGN.md
// "Judge summary and parameter sweeps").
//
// What one scene contributes (scene_part), how two contributions combine (merge: integers, minima
// and maxima, all independent of order), the 256-entry summation tree (tree256) and the histogram bin
// (hist_bin), compiled for the device (k_summary_tiles, k_summary_groups) and the host
// (pp_judge_summary_host, summarize_host below). The two FP64 sums are one fixed expression: per
// 256-scene tile of a group a pairwise tree, the tiles' results dealt round-robin onto 256 running
// sums in ascending tile order, then the same tree over those. Only + on the same operands in the same
// order, under -ffp-contract=off on both sides, so host and device agree bit for bit.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "../../include/pp.h"

#ifndef PP_HD
#define PP_HD __host__ __device__
#endif

namespace ppsummary {

constexpr int kTile = 256;                 // scenes per tile, entries of the tree
constexpr uint32_t kNoStep = 0xFFFFFFFFu;  // first-step minimum of a part without a violation

// What a scene, a tile or a group contributes to a row. A tile's record in the stream's workspace
// is one of these.
struct Part {
    double dist_sum, clean_sum;            // (a scene's own value, then tree256 results)
    double clean_min, clean_max, min_sep, max_mph, max_acc, max_jerk;
    int64_t n_unjudged, n_nonfinite, n_clean, steps;
    int64_t with[PP_INC_KINDS], steps_in[PP_INC_KINDS];
    uint32_t first[PP_INC_KINDS];          // smallest first_step > 0, kNoStep: none
    int32_t bin;                           // a scene's histogram bin, -1: not counted
};

PP_HD inline bool finite_(double x) { return x - x == 0; }     // neither NaN nor infinite
PP_HD inline double min_(double a, double b) { return b < a ? b : a; }
PP_HD inline double max_(double a, double b) { return b > a ? b : a; }

// The bin of a finite clean_dist: [0, hist_max) in B equal bins, the last one also holding what lies
// beyond (and the first what lies below 0, which the judge never produces).
PP_HD inline int hist_bin(double clean, double inv_w, int B) {
    const double q = clean * inv_w;
    return q >= B - 1 ? B - 1 : (q > 0 ? (int)q : 0);
}

// the part of nothing: what an unjudged scene, a lane past the group's end or an empty tile counts as
PP_HD inline void part_none(Part& p) {
    p.dist_sum = 0.0; p.clean_sum = 0.0;
    p.clean_min = INFINITY; p.clean_max = -INFINITY; p.min_sep = INFINITY;
    p.max_mph = -INFINITY; p.max_acc = -INFINITY; p.max_jerk = -INFINITY;
    p.n_unjudged = 0; p.n_nonfinite = 0; p.n_clean = 0; p.steps = 0;
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) { p.with[k] = 0; p.steps_in[k] = 0; p.first[k] = kNoStep; }
    p.bin = -1;
}

// scene s of a state of S scenes (only read)
PP_HD inline void scene_part(const pp_judge& st, int64_t S, int64_t s, double inv_w, int B, Part& p) {
    // every array is read before anything is decided (an unjudged scene's words are garbage, not
    // absent): the sixteen loads of a lane are in flight together, and what follows is selects
    const int32_t steps = st.steps[s];
    const uint32_t flags = st.flags[s];
    int32_t c[PP_INC_KINDS], f[PP_INC_KINDS];
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) { c[k] = st.count[(int64_t)k * S + s]; f[k] = st.first_step[(int64_t)k * S + s]; }
    const double dist = st.dist[s], clean = st.clean_dist[s];
    const double sep = st.min_sep[s], mph = st.max_speed_mph[s], acc = st.max_acc[s], jerk = st.max_jerk[s];
    const bool judged = steps != 0;
    const bool fin = judged && finite_(dist) && finite_(clean);
    p.n_unjudged = judged ? 0 : 1;
    p.n_nonfinite = judged && !fin ? 1 : 0;
    p.n_clean = judged && flags == 0 ? 1 : 0;
    p.steps = judged ? steps : 0;
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) {
        p.with[k] = judged && c[k] > 0 ? 1 : 0;
        p.steps_in[k] = judged ? c[k] : 0;
        p.first[k] = judged && f[k] > 0 ? (uint32_t)f[k] : kNoStep;
    }
    p.dist_sum = fin ? dist : 0.0;
    p.clean_sum = fin ? clean : 0.0;
    p.clean_min = fin ? clean : INFINITY;
    p.clean_max = fin ? clean : -INFINITY;
    p.bin = fin ? hist_bin(clean, inv_w, B) : -1;
    p.min_sep = judged && sep == sep ? sep : INFINITY;        // NaN ignored
    p.max_mph = judged && mph == mph ? mph : -INFINITY;
    p.max_acc = judged && acc == acc ? acc : -INFINITY;
    p.max_jerk = judged && jerk == jerk ? jerk : -INFINITY;
}

// a += b for everything but the two sums and the bin
PP_HD inline void merge(Part& a, const Part& b) {
    a.clean_min = min_(a.clean_min, b.clean_min); a.clean_max = max_(a.clean_max, b.clean_max);
    a.min_sep = min_(a.min_sep, b.min_sep);
    a.max_mph = max_(a.max_mph, b.max_mph); a.max_acc = max_(a.max_acc, b.max_acc);
    a.max_jerk = max_(a.max_jerk, b.max_jerk);
    a.n_unjudged += b.n_unjudged; a.n_nonfinite += b.n_nonfinite; a.n_clean += b.n_clean; a.steps += b.steps;
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) {
        a.with[k] += b.with[k]; a.steps_in[k] += b.steps_in[k];
        a.first[k] = b.first[k] < a.first[k] ? b.first[k] : a.first[k];
    }
}

// row `row` of stats arrays of R rows from a group's part (the histogram is not part of it)
PP_HD inline void write_row(const pp_judge_stats& o, int64_t R, int64_t row, int64_t n_scenes, const Part& p) {
    o.n_scenes[row] = n_scenes;
    o.n_unjudged[row] = p.n_unjudged; o.n_nonfinite[row] = p.n_nonfinite; o.n_clean[row] = p.n_clean;
    o.steps[row] = p.steps;
#pragma unroll
    for (int k = 0; k < PP_INC_KINDS; k++) {
        o.scenes_with[k * R + row] = p.with[k]; o.steps_in[k * R + row] = p.steps_in[k];
        o.first_step_min[k * R + row] = p.first[k] == kNoStep ? 0 : (int32_t)p.first[k];
    }
    o.dist_sum[row] = p.dist_sum; o.clean_dist_sum[row] = p.clean_sum;
    o.clean_dist_min[row] = p.clean_min; o.clean_dist_max[row] = p.clean_max;
    o.min_sep[row] = p.min_sep;
    o.max_speed_mph[row] = p.max_mph; o.max_acc[row] = p.max_acc; o.max_jerk[row] = p.max_jerk;
}

// groups of a state of S scenes, E per group; tiles of a group of n scenes
PP_HD inline int64_t n_groups(int64_t S, int64_t E) { return S / E + (S % E != 0 ? 1 : 0); }
PP_HD inline int64_t n_tiles(int64_t n) { return (n + kTile - 1) / kTile; }

inline bool stats_ok(const pp_judge_stats* o) {
    return o && o->n_scenes && o->n_unjudged && o->n_nonfinite && o->n_clean && o->steps && o->scenes_with &&
           o->steps_in && o->first_step_min && o->dist_sum && o->clean_dist_sum && o->clean_dist_min &&
           o->clean_dist_max && o->min_sep && o->max_speed_mph && o->max_acc && o->max_jerk && o->hist;
}

// every check of a summary configuration against a state of S scenes (the state's and the stats'
// pointers are the caller's to check)
inline bool cfg_ok(const pp_summary_cfg& c, int64_t S) {
    if (S < 0 || c.scenes_per_group < 1 || c.hist_bins < 1 || c.hist_bins > PP_STATS_MAX_BINS) return false;
    if (!finite_(c.hist_max) || !(c.hist_max > 0) || c.out_first < 0) return false;
    if (c.out_stride == 0) return c.out_first == 0;
    const int64_t G = n_groups(S, c.scenes_per_group);
    return c.out_stride >= G && c.out_first <= c.out_stride - G;
}

// ---- host only ----------------------------------------------------------------------------------
// tree256 as the definition states it: v[i] += v[i + w] for i < w, w = 128, 64, ..., 1
inline double tree256(double* v) {
    for (int w = kTile / 2; w >= 1; w >>= 1)
        for (int i = 0; i < w; i++) v[i] = v[i] + v[i + w];
    return v[0];
}

// The host twin's body: the definition evaluated group by group, tile by tile (arguments checked by
// the caller).
inline void summarize_host(const pp_judge& st, int64_t S, const pp_summary_cfg& c, const pp_judge_stats& o) {
    const int64_t E = c.scenes_per_group, G = n_groups(S, E);
    const int64_t R = c.out_stride ? c.out_stride : G;
    const int B = c.hist_bins;
    const double inv_w = B / c.hist_max;
    for (int64_t g = 0; g < G; g++) {
        const int64_t row = c.out_first + g, s0 = g * E, n = (S - s0 < E) ? S - s0 : E;
        for (int b = 0; b < B; b++) o.hist[b * R + row] = 0;
        Part grp;
        part_none(grp);
        double ud[kTile], uc[kTile];
        for (int i = 0; i < kTile; i++) { ud[i] = 0.0; uc[i] = 0.0; }
        for (int64_t t = 0; t < n_tiles(n); t++) {
            double vd[kTile], vc[kTile];
            for (int i = 0; i < kTile; i++) {
                const int64_t k = t * kTile + i;
                Part p;
                if (k < n) scene_part(st, S, s0 + k, inv_w, B, p); else part_none(p);
                vd[i] = p.dist_sum; vc[i] = p.clean_sum;
                merge(grp, p);
                if (p.bin >= 0) o.hist[p.bin * R + row]++;
            }
            const double Td = tree256(vd), Tc = tree256(vc);
            ud[t % kTile] = ud[t % kTile] + Td;
            uc[t % kTile] = uc[t % kTile] + Tc;
        }
        grp.dist_sum = tree256(ud);
        grp.clean_sum = tree256(uc);
        write_row(o, R, row, n, grp);
    }
}

}  // namespace ppsummary
