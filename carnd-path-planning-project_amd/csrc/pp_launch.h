// pp_launch.h — host: workspace sizing, launch-shape choices and pp_eval's launch sequences.
// Part of pp_eval.hip's translation unit.
#pragma once

namespace {

size_t prep_bytes(int64_t S) { return ((size_t)S * (kPrepD * 8 + kPrepI * 4) + 255) / 256 * 256; }
// reference-mode winner record (k_cand -> k_emit): 3 x PP_MAX_POINTS x S doubles + 2 x S u64
size_t rec_bytes(int64_t S) { return (size_t)S * (3 * PP_MAX_POINTS + 2) * 8 + 256; }
static_assert(kWinRec <= 3 * PP_MAX_POINTS + 2, "the stored winner slots share the record's memory");
double* rec_buf(void* rec) { return (double*)rec; }
uint64_t* adj_buf(void* rec, int64_t cap) { return (uint64_t*)((double*)rec + 3 * PP_MAX_POINTS * cap); }

PrepV prep_bind(void* base, int64_t S) {
    PrepV p;
    double* d = (double*)base;
    double** dd[] = {&p.pos_x, &p.pos_y, &p.angle, &p.ca_m, &p.sa_m, &p.ca_p, &p.sa_p,
                     &p.ego_speed, &p.ego_d, &p.ego_vd, &p.in_ts, &p.in_tt};
    int k = 0;
    for (double** q : dd) *q = d + (int64_t)(k++) * S;
    p.ratio = d + (int64_t)(k) * S; k += NL;
    p.l_ts = d + (int64_t)(k) * S; k += NL;
    p.l_tt = d + (int64_t)(k) * S; k += NL;
    p.score = d + (int64_t)(k) * S; k += NL;
    // k == kPrepD
    int32_t* ip = (int32_t*)(d + (int64_t)kPrepD * S);
    int32_t** ii[] = {&p.K, &p.ref_wp, &p.T, &p.ego_lane, &p.open_mask, &p.lim_mask, &p.status};
    int m = 0;
    for (int32_t** q : ii) *q = ip + (int64_t)(m++) * S;
    return p;
}

// pp_debug_set's switches (include/pp.h PP_DBG_*): launch-shape overrides for tests and A/B
// measurements. Every one defaults to 0 = the product's own choice; nothing reads the environment.
std::atomic<int> g_dbg[PP_DBG_KEYS];
int dbg(int key) { return g_dbg[key].load(std::memory_order_relaxed); }

// small reference-mode batches (<= kFusedSmall scenes): K2 + K4 in one launch (k_cand_small) or the
// whole step in one launch (k_step_small); PP_DBG_SHAPE forces one of the three shapes
constexpr int64_t kFusedSmall = 16384;
bool fused_small(int64_t S) {
    const int f = dbg(PP_DBG_SHAPE);
    return f ? f != PP_SHAPE_SPLIT : S <= kFusedSmall;
}
bool step_fused_on() { return dbg(PP_DBG_SHAPE) != PP_SHAPE_CAND_SMALL; }
// Two-stream split (reference mode, no paths): batches of about one 8-GPU shard of BASELINE config 5
// (262,144 scenes) run as two halves, each K1 -> K2 -> K4 on its own stream, so one half's kernels
// fill the other's start-up and tail (a batch this size is ~15 rounds of k_cand blocks and one of
// k_prep waves). Up to config 5's N = 2 shard (1,048,576 scenes: 4.96-4.99 ms against
// 5.09-5.15 unsplit, same boxes); the full 2,097,152-scene batch stays one stream (9.87-9.91 against
// 9.93-9.96 ms split, within the boxes' spread, and its K2 span is 0.3 ms longer than the unsplit
// K2). PP_DBG_SPLIT 1 forces it for every batch the split can take (reference mode without paths
// or draws, one K1 lane per scene: more than 65,536 scenes, prep_group), 2 turns it off; the parts
// of the last call are read back with PP_DBG_LAST_PARTS.
constexpr int64_t kSplitMin = 131072, kSplitMaxScenes = 1572864;
constexpr int64_t kChunkScenes = 1048576;
bool split_on(int64_t S) {
    const int f = dbg(PP_DBG_SPLIT);
    if (f == 2) return false;
    // forced: any batch of at least 2,048 scenes (its parts then never come out empty)
    if (f == 1) return S >= 2048;
    return S >= kSplitMin && S <= kSplitMaxScenes;
}
// parts of a split batch: 2 up to 393,216 scenes (BASELINE config 5's N = 8 shard, 262,144: 1.32 ms
// against 1.35 / 1.37 ms with 3 / 4 parts), 3 beyond (its N = 4 shard, 524,288: 2.52 ms against
// 2.59-2.62 with 2 parts and 2.60 unsplit; profiles/r04_ablations.txt)
int split_parts(int64_t S) {
    return S > 393216 ? 3 : 2;
}
// chunks of a split batch: a batch beyond kSplitMaxScenes, when split (PP_DBG_SPLIT 1),
// runs as ceil(S / 1,048,576) sequential chunks of split_parts parts each
// (chunk c + 1 starts when every part of chunk c has ended). Round 6 measured it for BASELINE
// config 5 (2,097,152 scenes; tools/chunk_probe.py, profiles/r06_chunk_probe*.txt): two separate
// pp_eval calls of 1,048,576 scenes (their own arrays) ran 9.78-9.87 ms against 9.79-9.99 for
// one call on one stream, but the same chunks inside one call (the batch's own arrays) ran
// 9.98-10.01 on the box where the separate calls took 9.85, and 6 parts pipelined over the 3
// streams without the join 10.00-10.07: the full batch stays on one stream.
int split_chunks(int64_t S) {
    if (S <= kSplitMaxScenes) return 1;
    const int64_t c = (S + kChunkScenes - 1) / kChunkScenes;
    return (int)std::min<int64_t>(c, kPartMax / kSplitMax);
}
// The persistent K2 (k_cand<Persist, 1>: reference mode without paths or draws, one stream): the
// batches beyond the split's range, where the grid is ~120 rounds of blocks and the dispatcher's
// refill of a block slot (~5 us after a ~64 us block) is what the step still pays beside its
// arithmetic (2,097,152 scenes: step 9.73-9.85 -> 9.47-9.60 ms, k_cand 7.29-7.33 -> 7.01-7.03).
// Measured against the split (profiles/persist_ablations.txt): slower at 262,144 and 524,288
// scenes (+1.3 / +1.0 %), level at 1,048,576, 2.5 % faster at 1,572,864, so the split keeps its
// range. PP_DBG_PERSIST 1 forces it for every batch launch_plain runs with the k_cand pair, 2
// turns it off; the last call's resident block count is read back with PP_DBG_LAST_PERSIST.
constexpr int64_t kPersistMinScenes = kSplitMaxScenes + 1;
bool persist_on(int64_t S) {
    const int f = dbg(PP_DBG_PERSIST);
    return f == 1 || (f == 0 && S >= kPersistMinScenes);
}
// K1 (one lane per evaluation): 3 waves per SIMD, or 4 where the batch's waves fill whole rounds of
// 4 better. Round 5 (the approach table in the 3-wave build's LDS): a round of 3 waves per SIMD
// takes ~0.150 ms (config 5: 1.65 ms for 32,768 waves = 11 rounds), one of 4 ~0.357 ms (spills,
// the table in global memory); 262,144 scenes = 4,096 waves: 0.297 ms at 3, 0.357 at 4
// (profiles/r05_ablations.txt), so the 4-wave build no longer wins at any size (round 4: 0.188 /
// 0.286 ms per round, 4 waves at 262,144). PP_DBG_PREP_WAVES forces 3 or 4.
int cu_count(int device) {
    static int cus[kMaxDev] = {};
    if (device < 0 || device >= kMaxDev) return 256;
    if (cus[device] == 0) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c <= 0) c = 256;
        cus[device] = c;
    }
    return cus[device];
}
// the one-launch step with phase A beside K1 (wave_step_body) where its blocks fit one per CU:
// 8-scene blocks of 256 threads (the frame, batches up to 2,048 scenes: 0.128 -> 0.116 ms at 2,048),
// else 16-scene blocks of 512 threads; beyond, 16-scene blocks of 256 threads, K1 then phase A
// (2 blocks of 8 per CU measured slower: config 2 0.132 against 0.128 ms, profiles/r04_ablations.txt)
int step_waves_on(int64_t S, int spb, int device) {
    if ((S + kStepWaveSpb - 1) / kStepWaveSpb <= cu_count(device)) return 1;
    if (spb >= 16 && (S + 15) / 16 <= cu_count(device)) return 2;
    return 0;
}
bool prep_w4(int64_t Sv, int device) {
    const int f = dbg(PP_DBG_PREP_WAVES);
    if (f == 3 || f == 4) return f == 4;
    const int64_t waves = (Sv + 63) / 64, simds = 4LL * cu_count(device);
    const int64_t r3 = (waves + 3 * simds - 1) / (3 * simds), r4 = (waves + 4 * simds - 1) / (4 * simds);
    return 357 * r4 < 150 * r3;
}
// k_emit: batches up to this many scenes take the small-batch instantiation
constexpr int64_t kEmitSmall = 65536;
// K1 lanes per evaluation: the largest power of two <= 16 that keeps Sv * G within ~2 waves per
// SIMD of the chip (256 CUs x 4 SIMDs x 64 lanes x 2); 1 for large batches. PP_DBG_PREP_GROUP
// forces a value.
bool prep_group_ok(int G) { return G == 0 || G == 1 || G == 2 || G == 4 || G == 8 || G == 16; }
int prep_group(int64_t Sv) {
    const int forced = dbg(PP_DBG_PREP_GROUP);
    if (forced > 0) return forced;
    const int64_t target = 256LL * 4 * 64 * 2;
    int G = 1;
    while (G < 16 && Sv * G * 2 <= target) G *= 2;
    return G;
}

// Scenes per k_cand group (C <= 256): at most 256 / C (one 256-lane block) and 64 / NL (spline
// slots: phase A's serial steps run on one wave), chosen so the block's waves carry the fewest
// idle lanes through phase B (largest such count on ties): C = 15 -> 17 scenes (255 of 256
// lanes), C = 24 (config 3) -> 8 scenes in exactly 3 waves instead of 10 in 4 waves with 16 idle
// lanes.
int cands_per_block(int C) {
    int hi = 256 / C;
    if (hi > 64 / NL) hi = 64 / NL;
    if (hi < 1) return 1;
    int best = hi;
    double bu = 0;
    for (int spb = hi; spb >= 1; spb--) {
        const int t = spb * C;
        const double u = (double)t / (double)(((t + 63) / 64) * 64);
        if (u > bu + 1e-9) { bu = u; best = spb; }
    }
    return best;
}

// callers hold M->mu; `st` is the stream the workspace belongs to (DevMem::grow drains it before
// a buffer is replaced)
int ensure_ws(StreamWS& W, hipStream_t st, int64_t Sv) { return W.ws.grow(st, Sv, prep_bytes(Sv)); }

// k_sort_cars' output for S scenes of `rows` rows each (SortedCars over one allocation)
size_t srt_bytes(int64_t S, int rows) { return (size_t)S * ((size_t)rows * (4 * sizeof(double) + sizeof(int)) + 8) + 256; }
int ensure_srt(StreamWS& W, hipStream_t st, int64_t S, int rows, SortedCars& sc) {
    const size_t need = srt_bytes(S, rows);
    const int rc = W.srt.grow(st, (int64_t)need, need);
    if (rc) return rc;
    double* b = (double*)W.srt.get();
    const int64_t n = (int64_t)rows * S;
    sc.x = b; sc.y = b + n; sc.vx = b + 2 * n; sc.vy = b + 3 * n;
    sc.id = (int*)(b + 4 * n);
    sc.order = (uint64_t*)(((uintptr_t)(sc.id + n) + 7) & ~(uintptr_t)7);
    sc.rows = rows;
    return PP_OK;
}

int ensure_rec(StreamWS& W, hipStream_t st, int64_t S) {
    const int64_t cap = (S + 63) & ~(int64_t)63;   // whole 64-scene blocks
    return W.rec.grow(st, cap, rec_bytes(cap));
}

// The slow-group bitmap (words), then the flagged-group count and list (ngroups entries), in one
// allocation: [cap words][count][list: 32 cap entries]
int ensure_gbits(StreamWS& W, hipStream_t st, int64_t ngroups) {
    const int64_t words = (ngroups + 31) / 32;
    if (W.gbits.cap() >= words) return PP_OK;
    const int64_t cap = std::max<int64_t>(words, 1024);
    // [bits: cap words][the parts' flagged-group counts: kPartMax words][the persistent kernels'
    // claim counters: kPersistCtr words][list: 32 cap entries]
    const size_t bytes = sizeof(uint32_t) * (size_t)(cap + kPartMax + kPersistCtr + 32 * cap);
    DevMem<uint32_t> g = std::move(W.gbits);       // (back only once it is cleared)
    const int rc = g.grow(st, cap, bytes);
    if (rc) return rc;
    if (hipMemsetAsync(g.get(), 0, bytes, st) != hipSuccess) return PP_ERR_HIP;
    W.gbits = std::move(g);
    return PP_OK;
}

// k_cand's launch geometry for C candidates per scene (BPS == 1: SPB scenes per group; else one
// scene over BPS groups of 256 candidates)
// (lds: the block's LDS without the cost array, CandLds)
struct CandGeom { int spb, bps, threads; size_t lds; int64_t groups; };
// the flat geometry for the all-paths mode (kMode 2): 256-lane groups over the batch's candidates,
// scenes straddling two groups (their spline slots built in both, status flags merged with
// atomics): four full waves per block where whole scenes would leave a wave slot of the CU idle
// (C = 24: 8 scenes in 3 waves, 5 blocks = 15 of 16 waves per CU). Up to (C + 254) / C + 1 scenes
// per group; C >= 13 keeps those slots within the first wave (NL SPB <= 64 for phase A's serial steps)
bool cand_flat_ok(int C) { return C >= 13 && C <= 128 && 256 % C != 0; }
CandGeom cand_geom(int C, int64_t S, bool flat = false) {
    CandGeom g;
    if (flat) {
        g.spb = (C + 254) / C + 1;
        g.bps = -1;
        g.threads = 256;
        g.lds = CandLds{g.spb}.bytes();
        g.groups = (S * C + 255) / 256;
        return g;
    }
    g.spb = C <= 256 ? cands_per_block(C) : 1;
    g.bps = C <= 256 ? 1 : (C + 255) / 256;
    g.threads = C <= 256 ? ((g.spb * C + 63) / 64) * 64 : 256;
    g.lds = CandLds{g.spb}.bytes();
    g.groups = g.bps == 1 ? (S + g.spb - 1) / g.spb : S * g.bps;
    return g;
}

int n_draws(const pp_params* p) { return p->n_draws > 1 ? p->n_draws : 1; }

// k_prep<true, false>'s LDS with the approach table after the map (MapG::atab_lds)
size_t prep_lds_atab(int n) {
    return sizeof(double) * (((kMapArrays * (size_t)n + 1) & ~(size_t)1) + kAtabD * (size_t)n);
}

bool params_ok(const pp_params* p) {
    return p && p->n_points > PP_PREV_KEEP && p->n_points <= PP_MAX_POINTS && p->n_speeds >= 1 &&
           p->n_speeds <= PP_MAX_SPEEDS && NL * p->n_speeds <= 256 &&
           (p->cost_mode == PP_COST_REFERENCE || p->cost_mode == PP_COST_COMFORT) &&
           p->n_draws >= 0 && p->n_draws <= PP_MAX_DRAWS && p->noise_first_scene >= 0 &&
           !(p->n_draws > 1 && p->emit_paths);
}

// ---- pp_eval in steps: the argument check, the call's plan, its workspace and kernel arguments
// (bound under M->mu), then one of three launch sequences (launch_step, launch_split, launch_plain)

// (a batch of no scenes passes without its arrays: the caller returns PP_OK for it)
int32_t eval_check(const pp_map* M, const pp_scene_batch* in, const pp_params* prm, const pp_result* out,
                   int32_t device) {
    if (!M || !in || !out || !params_ok(prm) || device < 0 || device >= kMaxDev) return PP_ERR_ARG;
    if (in->n_scenes < 0 || in->car_stride < 0 || in->car_stride > PP_MAX_CARS) return PP_ERR_ARG;
    if (in->n_scenes == 0) return PP_OK;
    if (!in->ego_x || !in->ego_y || !in->ego_yaw_deg || !in->ego_speed_mph || !in->prev_x ||
        !in->prev_y || !in->n_prev || !in->prev_target_lane || !in->n_cars ||
        (in->car_stride > 0 && (!in->car_id || !in->car_x || !in->car_y || !in->car_vx || !in->car_vy)))
        return PP_ERR_ARG;
    if (!out->winner || !out->n_out || !out->next_x || !out->next_y || !out->cost || !out->status)
        return PP_ERR_ARG;
    if (prm->emit_paths && !out->paths) return PP_ERR_ARG;
    if (in->tab_valid && (!in->tab_lane || !in->tab_s || !in->tab_d || !in->tab_vs || !in->tab_vd ||
                          !in->tab_vx || !in->tab_vy || prm->n_draws > 1 || in->tab_slots < 0 ||
                          in->tab_slots > PP_MAX_CARS))
        return PP_ERR_ARG;
    return PP_OK;
}

// The call's plan: which launch sequence it takes and what that needs (eval_plan: no launch, no
// allocation)
struct EvalPlan {
    int64_t S, Sv;            // scenes; evaluations (scene x draw)
    int Dn, Cn;               // draws (>= 1); candidates per scene (draws x lanes x speeds)
    // reference decision without draws: the winner is known before the loop (k_cand records it,
    // k_emit writes it); otherwise the decision is a cost argmin (k_winner)
    bool ref_direct;
    CandGeom cg;
    // small batches in reference mode without paths: K2 and K4 in one launch (k_cand_small, K4 in
    // the block), unless the horizon's sin/cos table (2 N doubles per winner) exceeds the
    // block's spline slots. Large batches keep K4 in its own kernel: in the block, the serial
    // replay holds the block's LDS and costs k_cand more than k_emit takes.
    bool fused;
    // small reference-mode batches with the map in LDS: the whole step in one launch (k_step_small)
    // (step_waves: blocks of up to kStepWaveSpb scenes in 256 threads, K1 and phase A side by side,
    // plus the per-scene geometry records; otherwise up to 16 scenes, K1 then phase A)
    // step_waves: 1 blocks of 8 scenes in 256 threads, 2 blocks of 16 scenes in 512 threads, 0 the
    // 16-scene blocks without the split
    int step_waves, spb_f;
    int64_t groups_f;
    size_t lds_f;
    bool step_fused;
    int prep_g;               // K1 lanes per evaluation (prep_group)
    bool need_rec;            // the winner record (k_cand -> k_emit, or inside the fused kernels)
    // comfort mode without paths or draws, every scene's candidates in one block: k_cand makes the
    // decision and stores the winner's spline slot in the record's memory (kWinRec x 8 = 624 B per scene of its
    // 3,088), k_winner_st re-runs the winner from it
    bool need_wslot;
    // K0 (k_sort_cars) ahead of the one-lane K1: no car table, fewer than kSortDmax draws, at
    // most 16 rows per scene (k_prep's own sorting rule; larger tables keep the identity order)
    bool need_srt;
    bool split;               // the multi-stream split (split_on)
    bool persist;             // the persistent K2 in place of k_cand<false> (persist_on)
};
int32_t eval_plan(const pp_map* M, const pp_scene_batch* in, const pp_params* prm, int32_t device, EvalPlan& p) {
    p.S = in->n_scenes;
    p.Dn = n_draws(prm);
    p.Sv = p.S * p.Dn;
    p.ref_direct = prm->cost_mode == PP_COST_REFERENCE && p.Dn == 1;
    p.Cn = p.Dn * NL * prm->n_speeds;
    p.cg = cand_geom(p.Cn, p.S, prm->emit_paths && p.Dn == 1 && cand_flat_ok(p.Cn));
    if (p.cg.groups > 0x7fffffff) return PP_ERR_ARG;
    p.fused = p.ref_direct && !prm->emit_paths && p.cg.bps == 1 && CandLds{p.cg.spb}.replay_fits(prm->n_points) && fused_small(p.S);
    p.step_waves = step_waves_on(p.S, p.cg.spb, device);
    const size_t map_lds = sizeof(double) * (size_t)((kMapArrays * M->n + 1) & ~1);
    auto step_lds = [&](int wv, int spb) {
        return map_lds + (wv != 0 ? sizeof(double) * (size_t)(CandLds{spb}.doubles() + kGeoD * spb) : CandLds{spb}.bytes());
    };
    if (p.step_waves && step_lds(p.step_waves, std::min(p.cg.spb, p.step_waves == 1 ? kStepWaveSpb : 16)) > 65536) p.step_waves = 0;
    p.spb_f = std::min(p.cg.spb, p.step_waves == 1 ? kStepWaveSpb : 256 / 16);
    p.groups_f = (p.S + p.spb_f - 1) / p.spb_f;
    p.lds_f = step_lds(p.step_waves, p.spb_f);
    p.step_fused = p.fused && M->n <= kLdsMapMax && p.lds_f <= 65536 && step_fused_on();
    p.prep_g = prep_group(p.Sv);
    p.need_rec = p.ref_direct && !prm->emit_paths;
    p.need_wslot = !p.ref_direct && !prm->emit_paths && p.cg.bps == 1 && p.Dn == 1;
    p.need_srt = dbg(PP_DBG_SORT_CARS) == 1 && !in->tab_valid && p.Dn < kSortDmax && in->car_stride >= 2 &&
                 in->car_stride <= 16 && p.prep_g == 1;
    p.split = p.ref_direct && !prm->emit_paths && !p.fused && p.cg.bps == 1 && p.Dn == 1 && p.prep_g == 1 &&
              split_on(p.S);
    p.persist = p.ref_direct && !prm->emit_paths && !p.fused && !p.split && p.cg.bps == 1 && p.Dn == 1 &&
                persist_on(p.S);
    return PP_OK;
}

// What the call's launches pass: the stream, the kernels' arguments and the workspace behind them
struct EvalArgs {
    hipStream_t st;
    int32_t device;
    MapG mg;
    pp_scene_batch B;
    pp_params P;
    pp_result R;
    PrepV pv;
    GroupBits gb = {};
    double* rec = nullptr;    // the winner record and its adjusted-step masks (null: not in use)
    uint64_t* adjm = nullptr;
    double* wslot = nullptr;  // the stored winner slots (null: not in use)
    size_t cand_lds;          // k_cand's dynamic LDS
    SortedCars srt = {};      // rows 0: not in use
    uint32_t* next = nullptr; // the persistent kernels' claim counters (kPersistCtr words, zero before K1)
    unsigned persist = 0;     // the persistent k_cand's blocks (0: the call takes k_cand<false>)
    bool persist_shape = false;   // ... in the instantiation with config 5's shape as constants (cand_group's kShape)
};

// the stream's workspace at the call's size, then every argument of the call's launches: A is
// complete when this returns (callers hold M->mu)
int32_t eval_bind(const pp_map* M, const DevState& DS, StreamWS& W, const pp_scene_batch* in,
                  const pp_params* prm, const pp_result* out, int32_t device, void* hip_stream,
                  const EvalPlan& p, EvalArgs& A) {
    A.st = (hipStream_t)hip_stream;
    A.device = device;
    int rc = ensure_ws(W, A.st, p.Sv);
    if (rc) return rc;
    rc = ensure_gbits(W, A.st, p.cg.groups);
    if (rc) return rc;
    if (p.need_rec) {
        rc = ensure_rec(W, A.st, p.S);
        if (rc) return rc;
        A.rec = rec_buf(W.rec.get());
        A.adjm = adj_buf(W.rec.get(), W.rec.cap());
    }
    if (p.need_srt) {
        rc = ensure_srt(W, A.st, p.S, in->car_stride, A.srt);
        if (rc) return rc;
    }
    A.cand_lds = p.cg.lds;
    if (p.need_wslot) {
        rc = ensure_rec(W, A.st, p.S);
        if (rc) return rc;
        A.wslot = rec_buf(W.rec.get());
        A.cand_lds = CandLds{p.cg.spb}.bytes_cost();     // + sCost
    }
    A.pv = prep_bind(W.ws.get(), W.ws.cap());
    A.mg.buf = DS.tab.map.get();
    A.mg.n = M->n;
    A.mg.fastm = M->fastm;
    A.mg.wg = M->wg;
    A.mg.wg.cells = DS.tab.wgrid.get();
    A.mg.wseg = DS.tab.wseg.get();
    A.mg.atab = DS.tab.atab.get();
    // k_prep<true, false> stages the approach table after the map where both fit a block's 64 KB
    A.mg.atab_lds = DS.tab.atab && prep_lds_atab(M->n) <= 65536;
    A.P = *prm;
    A.B = *in;
    A.R = *out;
    if (!A.P.emit_paths) { A.R.paths = nullptr; A.R.path_len = nullptr; }
    A.gb.bits = W.gbits.get(); A.gb.SPB = p.cg.spb; A.gb.BPS = p.cg.bps; A.gb.C = p.Cn;
    A.gb.count = W.gbits.get() + W.gbits.cap();
    A.next = A.gb.count + kPartMax;
    A.gb.list = A.next + kPersistCtr;
    return PP_OK;
}

// PP_DBG_POISON: every call starts from NaN-filled (0xFF) intermediates and outputs, so no kernel can
// lean on what an earlier call left there (or on an output element it never writes); the
// slow-group bitmap must be all zero between calls (k_cand<true> clears what k_prep set)
int32_t poison_fill(const StreamWS& W, hipStream_t st, const EvalPlan& p, const pp_params* prm,
                    const pp_result* out) {
    auto fill = [&](void* q, size_t bytes) { return !q || !bytes || hipMemsetAsync(q, 0xFF, bytes, st) == hipSuccess; };
    const int64_t S = p.S, Cn = p.Cn, N = prm->n_points;
    const int64_t words = (p.cg.groups + 31) / 32;
    std::vector<uint32_t> hb((size_t)words);
    if (hipMemcpyAsync(hb.data(), W.gbits.get(), sizeof(uint32_t) * words, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PP_ERR_HIP;
    for (uint32_t w : hb)
        if (w) return PP_ERR_STATE;
    const bool ok = fill(W.ws.get(), prep_bytes(W.ws.cap())) &&
                    fill(W.rec.get(), W.rec ? rec_bytes(W.rec.cap()) : 0) &&
                    fill(W.srt.get(), (size_t)W.srt.cap()) &&
                    fill(W.gbits.get() + W.gbits.cap() + kPartMax + kPersistCtr, sizeof(uint32_t) * 32 * (size_t)W.gbits.cap()) &&
                    fill(out->winner, 4 * S) && fill(out->n_out, 4 * S) && fill(out->status, 4 * S) &&
                    fill(out->next_x, 8 * N * S) && fill(out->next_y, 8 * N * S) &&
                    fill(out->cost, 8 * Cn * S) && fill(out->info, sizeof(pp_scene_info) * S) &&
                    fill(out->draw_mean_cost, p.Dn > 1 ? 8 * NL * prm->n_speeds * S : 0) &&
                    fill(prm->emit_paths ? out->paths : nullptr, 16 * N * Cn * S) &&
                    fill(prm->emit_paths ? out->path_len : nullptr, 4 * Cn * S);
    return ok ? PP_OK : PP_ERR_HIP;
}

#ifdef PP_CHECK
// checking builds: the bounds of every buffer this call's kernels store into. g_lim is one record
// for the device, so the device is drained before it changes: a call of the same map still running
// on another stream (tests/test_concurrency.py) would otherwise be checked against this call's
// buffers. (Calls on different maps hold different locks: a checking build takes one map at a time.)
int32_t check_limits(const StreamWS& W, const EvalPlan& p, const EvalArgs& A) {
    ChkLim L = {};
    const long long Cn = p.Cn;
    L.paths = A.R.paths; L.npaths = A.R.paths ? (long long)p.S * A.P.n_points * Cn * 2 : 0;
    L.nx = A.R.next_x; L.ny = A.R.next_y; L.nnext = (long long)p.S * A.P.n_points;
    L.rec = A.rec; L.nrec = A.rec ? 3LL * PP_MAX_POINTS * W.rec.cap() : 0;
    L.adjm = (const unsigned long long*)A.adjm; L.nadj = A.adjm ? 2LL * W.rec.cap() : 0;
    L.cost = A.R.cost; L.ncost = (long long)p.S * Cn; L.nscen = p.S;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_lim), &L, sizeof L) != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}
#endif

// The call's timing record. tall: events at every kernel boundary; tk2: at K2's (PP_TIMING_K2
// records only those two). The record is a group of 4 kPartMax slots (before K1, after K1, after K2,
// after K3/K4, per part); a slot takes an event from the pool when it is first recorded (ev_at), so a
// K2-only call takes 2 events (2 per part when split) and an all-kernel call 4 per part
struct EvalEvents { DevState* DS; size_t base; bool timing, tall, tk2; };
hipEvent_t ev_at(const EvalEvents& E, int i) {
    DevState& DS = *E.DS;
    hipEvent_t& e = DS.ev.rec[E.base + i];
    if (!e) {
        if (DS.ev.pool.empty() && hipEventCreate(&e) != hipSuccess) return nullptr;
        if (!e) { e = DS.ev.pool.back(); DS.ev.pool.pop_back(); }
    }
    return e;
}

// The one-launch step (k_step_small, k_step_small512; fio: k_plan_frame)
int32_t launch_step(const EvalArgs& A, const EvalPlan& p, const EvalEvents& E, const FrameIO* fio) {
    hipStream_t st = A.st;
    if (E.timing) E.DS->ev.kind.back() |= 32;          // (no K1 kernel: K1 runs inside the step)
    if (E.tall) (void)hipEventRecord(ev_at(E, 0), st);
    // K1 takes 16 lanes for each of the block's spb_f scenes, K2 spb_f x C lanes: the block needs
    // both (C <= 9 gives cg.threads < 16 spb_f; the K1 of the scenes beyond would not run)
    const int threads_f = p.step_waves == 1 ? 256 : p.step_waves == 2 ? 512
                                                  : std::max(p.cg.threads, ((16 * p.spb_f + 63) / 64) * 64);
    // the step kernel's own start/end timestamps go into K2's events (the launch's dispatch
    // records them): no marker packets in the stream, which cost a few us each in a ~0.1 ms step
    hipEvent_t e1 = E.tk2 ? ev_at(E, 1) : nullptr, e2 = E.tk2 ? ev_at(E, 2) : nullptr;
    if (fio) {
        if (E.tk2) (void)hipEventRecord(ev_at(E, 1), st);
        hipLaunchKernelGGL(k_plan_frame, dim3(1), dim3(threads_f), p.lds_f, st, *fio, A.mg, A.B, A.P, A.pv, A.R, p.spb_f,
                           A.rec, A.adjm, p.step_waves == 1 ? 1 : 0);
        if (E.tk2) (void)hipEventRecord(ev_at(E, 2), st);
    } else if (p.step_waves == 2) {
        hipExtLaunchKernelGGL(k_step_small512, dim3((unsigned)p.groups_f), dim3(threads_f), (uint32_t)p.lds_f, st,
                              e1, e2, 0u, A.mg, A.B, A.P, A.pv, A.R, p.spb_f, A.rec, A.adjm);
    } else {
        hipExtLaunchKernelGGL(k_step_small, dim3((unsigned)p.groups_f), dim3(threads_f), (uint32_t)p.lds_f, st,
                              e1, e2, 0u, A.mg, A.B, A.P, A.pv, A.R, p.spb_f, A.rec, A.adjm, p.step_waves == 1 ? 1 : 0);
    }
    if (E.tall) (void)hipEventRecord(ev_at(E, 3), st);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

// The one-lane K1's launch: the map in LDS or in global memory, 3 or 4 waves per SIMD (prep_w4),
// the rows as given or sorted by K0 (srt.rows). lds_a and mga are k_prep<true, false>'s: the
// approach table staged after the map where both fit a block's 64 KB, else no table
struct PrepLds { bool lmap; size_t lds, lds_a; MapG mga; };
PrepLds prep_lds(const MapG& mg) {
    PrepLds L;
    L.lmap = mg.n <= kLdsMapMax;
    L.lds = L.lmap ? sizeof(double) * kMapArrays * (size_t)mg.n : 0;
    L.lds_a = L.lmap && mg.atab_lds ? prep_lds_atab(mg.n) : L.lds;
    L.mga = mg;
    if (!mg.atab_lds) L.mga.atab = nullptr;
    return L;
}
template <bool kW4, bool kK0>
void launch_prep_k(const EvalArgs& A, hipStream_t sh, int64_t v0, int64_t v1, const GroupBits& gb,
                   const SortedCars& srt, const PrepLds& L) {
    const unsigned pb = (unsigned)((v1 - v0 + 255) / 256);
    if (L.lmap) hipLaunchKernelGGL((k_prep<true, kW4, kK0>), dim3(pb), dim3(256), kW4 ? L.lds : L.lds_a, sh, kW4 ? A.mg : L.mga, A.B, A.P, A.pv, A.R.info, A.R.status, gb, v0, v1, srt);
    else hipLaunchKernelGGL((k_prep<false, kW4, kK0>), dim3(pb), dim3(256), 0, sh, A.mg, A.B, A.P, A.pv, A.R.info, A.R.status, gb, v0, v1, srt);
}
void launch_prep(const EvalArgs& A, hipStream_t sh, int64_t v0, int64_t v1, const GroupBits& gb,
                 const SortedCars& srt, const PrepLds& L) {
    const bool w4 = prep_w4(v1 - v0, A.device);
    if (srt.rows) {
        if (w4) launch_prep_k<true, true>(A, sh, v0, v1, gb, srt, L);
        else launch_prep_k<false, true>(A, sh, v0, v1, gb, srt, L);
    } else if (w4) {
        launch_prep_k<true, false>(A, sh, v0, v1, gb, srt, L);
    } else {
        launch_prep_k<false, false>(A, sh, v0, v1, gb, srt, L);
    }
}
// the grouped K1 (G lanes per evaluation): its LDS-map and global-map instantiations
using PrepGrpKernel = void (*)(MapG, pp_scene_batch, pp_params, PrepV, pp_scene_info*, uint32_t*, GroupBits);
void launch_prep_grp(PrepGrpKernel k_lds, PrepGrpKernel k_glob, const EvalArgs& A, int64_t blocks, const PrepLds& L) {
    if (L.lmap) hipLaunchKernelGGL(k_lds, dim3((unsigned)blocks), dim3(256), L.lds, A.st, A.mg, A.B, A.P, A.pv, A.R.info, A.R.status, A.gb);
    else hipLaunchKernelGGL(k_glob, dim3((unsigned)blocks), dim3(256), 0, A.st, A.mg, A.B, A.P, A.pv, A.R.info, A.R.status, A.gb);
}
// k_cand's pair: the fast instantiation over groups [g0, g0 + nb), then the checked one (nslow
// blocks) over the groups that K1 or the fast one flagged (their list and count)
template <int kMode>
void launch_cand(const EvalArgs& A, hipStream_t sh, const CandGeom& cg, unsigned nb, unsigned nslow,
                 uint32_t* list, uint32_t* count, int64_t g0) {
    hipLaunchKernelGGL((k_cand<false, kMode>), dim3(nb), dim3(cg.threads), A.cand_lds, sh, A.mg, A.B, A.P, A.pv, A.R,
                       cg.spb, cg.bps, A.rec, A.adjm, A.gb.bits, cg.groups, list, count, g0, A.wslot);
    hipLaunchKernelGGL((k_cand<true, kMode>), dim3(nslow), dim3(cg.threads), A.cand_lds, sh, A.mg, A.B, A.P, A.pv, A.R,
                       cg.spb, cg.bps, A.rec, A.adjm, A.gb.bits, cg.groups, list, count, g0, A.wslot);
}

// The multi-stream split (reference mode without paths or draws, one K1 lane per scene).
// NT = streams x chunks parts at group boundaries: part t takes groups [G t / NT, G (t + 1) /
// NT) and their scenes, on stream t % NS (stream 0: the caller's, else st2[.]); each part its
// own flagged-group list (count word t, its list from its first group's index on).
// Chunks run one after another (fork and join per chunk).
// Timing: each part's kernels by events on its own stream; pp_timing_read counts each stage
// once per call, as the span from a chunk's first part's start to its last part's end (the
// parts overlap, so one part's duration understates the stage's throughput), summed over
// the chunks.
int32_t launch_split(const EvalArgs& A, const EvalPlan& p, const EvalEvents& E, StreamWS& W) {
    hipStream_t st = A.st;
    const CandGeom& cg = p.cg;
    const int64_t S = p.S;
    const int NS = split_parts(S), NC = split_chunks(S), NT = NS * NC;
    if (!W.fork && hipEventCreateWithFlags(W.fork.out(), hipEventDisableTiming) != hipSuccess) return PP_ERR_HIP;
    for (int k = 0; k < NS - 1; k++)
        if ((!W.st2[k] && hipStreamCreateWithFlags(W.st2[k].out(), hipStreamNonBlocking) != hipSuccess) ||
            (!W.join[k] && hipEventCreateWithFlags(W.join[k].out(), hipEventDisableTiming) != hipSuccess))
            return PP_ERR_HIP;
    const int64_t G = cg.groups;
    const PrepLds L = prep_lds(A.mg);
    int launched = 0;     // parts launched (an empty part is skipped; never at >= 2,048 scenes)
    for (int c = 0; c < NC; c++) {
        // fork: the chunk's other streams start behind everything before it on the caller's stream
        if (hipEventRecord(W.fork.get(), st) != hipSuccess) return PP_ERR_HIP;
        for (int k = 0; k < NS - 1; k++)
            if (hipStreamWaitEvent(W.st2[k].get(), W.fork.get(), 0) != hipSuccess) return PP_ERR_HIP;
        for (int h = 0; h < NS; h++) {
            const int t = c * NS + h;
            hipStream_t sh = h == 0 ? st : W.st2[h - 1].get();
            const int64_t g0 = G * t / NT, g1 = G * (t + 1) / NT;
            const int64_t v0 = std::min<int64_t>(S, g0 * cg.spb), v1 = std::min<int64_t>(S, g1 * cg.spb);
            if (v1 <= v0) continue;
            GroupBits gbh = A.gb;
            gbh.count = A.gb.count + t;
            gbh.list = A.gb.list + g0;
            const int eh = 4 * launched++;
            if (E.tall) (void)hipEventRecord(ev_at(E, eh), sh);
            const unsigned pb = (unsigned)((v1 - v0 + 255) / 256);
            if (A.srt.rows)         // (the split takes batches without draws: scene = evaluation)
                hipLaunchKernelGGL(k_sort_cars, dim3(pb), dim3(256), 0, sh, A.B, A.srt, v0, v1);
            launch_prep(A, sh, v0, v1, gbh, A.srt, L);
            if (E.tk2) (void)hipEventRecord(ev_at(E, eh + 1), sh);
            const unsigned nsl = (unsigned)std::min<int64_t>(g1 - g0, 2048);
            launch_cand<1>(A, sh, cg, (unsigned)(g1 - g0), nsl, gbh.list, gbh.count, g0);
            if (E.tk2) (void)hipEventRecord(ev_at(E, eh + 2), sh);
            hipLaunchKernelGGL(k_emit<kEmitRows>, dim3(pb), dim3(256), 0, sh, A.B, A.P, A.pv, A.R,
                               A.rec, A.adjm, v0, v1);
            if (E.tall) (void)hipEventRecord(ev_at(E, eh + 3), sh);
        }
        // join: the caller's stream waits for the chunk's other streams
        for (int k = 0; k < NS - 1; k++)
            if (hipEventRecord(W.join[k].get(), W.st2[k].get()) != hipSuccess || hipStreamWaitEvent(st, W.join[k].get(), 0) != hipSuccess)
                return PP_ERR_HIP;
    }
    // (the timing record: parts launched, and parts per chunk for the per-chunk spans)
    if (E.timing) E.DS->ev.kind.back() |= (launched << 8) | (NC > 1 ? NS << 16 : 0);
    g_dbg[PP_DBG_LAST_PARTS].store(launched, std::memory_order_relaxed);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

// the persistent k_cand's grid: the blocks of this launch geometry that the device holds at once
// (the occupancy query, at most kCandWaves waves per SIMD, x CUs), asked once per device
unsigned persist_blocks(DevState& DS, const CandGeom& cg, int device) {
    const size_t lds = CandLds{cg.spb}.bytes_persist();
    if (DS.persist_blocks == 0 || DS.persist_threads != cg.threads || DS.persist_lds != lds) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_cand<Persist, 1>, cg.threads, lds) != hipSuccess || nb < 1) {
            (void)hipGetLastError();
            nb = 1;
        }
        nb = std::min(nb, std::max(1, 4 * kCandWaves * 64 / cg.threads));
        DS.persist_blocks = nb * cu_count(device);
        DS.persist_threads = cg.threads;
        DS.persist_lds = lds;
    }
    return (unsigned)DS.persist_blocks;
}

// One stream: K1 (after K0 where the rows are sorted), K2, then K4 or K3
int32_t launch_plain(const EvalArgs& A, const EvalPlan& p, const EvalEvents& E) {
    hipStream_t st = A.st;
    const CandGeom& cg = p.cg;
    const int64_t S = p.S, Sv = p.Sv;
    // K1: one lane per evaluation, or a group of G lanes per evaluation for small batches
    {
        const int G = p.prep_g;
        const int64_t blocks = (Sv * G + 255) / 256;
        if (E.tall) (void)hipEventRecord(ev_at(E, 0), st);
        const PrepLds L = prep_lds(A.mg);
        switch (G) {
            case 2: launch_prep_grp(k_prep_g2<true>, k_prep_g2<false>, A, blocks, L); break;
            case 4: launch_prep_grp(k_prep_g4<true>, k_prep_g4<false>, A, blocks, L); break;
            case 8: launch_prep_grp(k_prep_g8<true>, k_prep_g8<false>, A, blocks, L); break;
            case 16: launch_prep_grp(k_prep_g16<true>, k_prep_g16<false>, A, blocks, L); break;
            default:
                if (A.srt.rows)
                    hipLaunchKernelGGL(k_sort_cars, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, A.B, A.srt, (int64_t)0, S);
                launch_prep(A, st, 0, Sv, A.gb, A.srt, L);
                break;
        }
    }
    // K2 (+ K4 for small batches in reference mode: k_cand_small)
    {
        const unsigned nb = (unsigned)cg.groups;
        const unsigned nslow = (unsigned)std::min<int64_t>(cg.groups, 2048);
        if (E.tk2) (void)hipEventRecord(ev_at(E, 1), st);
        if (A.P.emit_paths) launch_cand<2>(A, st, cg, nb, nslow, A.gb.list, A.gb.count, 0);
        else if (p.ref_direct && p.fused) {
            hipLaunchKernelGGL(k_cand_small, dim3(nb), dim3(cg.threads), cg.lds, st, A.mg, A.B, A.P, A.pv, A.R,
                               cg.spb, A.rec, A.adjm, A.gb.bits);
        }
        else if (p.ref_direct && A.persist) {
            // resident blocks that claim their groups (at most one block per group), then the
            // checked instantiation over the flagged groups as after k_cand<false>
            const PersistArgs pa = {A.mg, A.B, A.P, A.pv, A.R, cg.spb, A.rec, A.adjm, cg.groups, A.next};
            // (config 5's shape takes the instantiation that has it as compile-time constants)
            if (A.persist_shape)
                hipLaunchKernelGGL((k_cand<PersistShape, 1>), dim3(std::min(A.persist, nb)), dim3(cg.threads),
                                   CandLds{cg.spb}.bytes_persist(), st, pa);
            else
                hipLaunchKernelGGL((k_cand<Persist, 1>), dim3(std::min(A.persist, nb)), dim3(cg.threads),
                                   CandLds{cg.spb}.bytes_persist(), st, pa);
            hipLaunchKernelGGL((k_cand<true, 1>), dim3(nslow), dim3(cg.threads), A.cand_lds, st, A.mg, A.B, A.P, A.pv, A.R,
                               cg.spb, cg.bps, A.rec, A.adjm, A.gb.bits, cg.groups, A.gb.list, A.gb.count, (int64_t)0, A.wslot);
        }
        else if (p.ref_direct) launch_cand<1>(A, st, cg, nb, nslow, A.gb.list, A.gb.count, 0);
        else launch_cand<0>(A, st, cg, nb, nslow, A.gb.list, A.gb.count, 0);
    }
    if (E.tk2) (void)hipEventRecord(ev_at(E, 2), st);
    // K4 (reference mode, winner-only output): replay the winners' recorded paths
    if (p.ref_direct && !A.P.emit_paths && !p.fused) {
        if (S <= kEmitSmall) {     // latency regime: 64-lane blocks over more CUs, 16 steps per load round
            const int64_t blocks = (S + 63) / 64;
            hipLaunchKernelGGL(k_emit<16>, dim3((unsigned)blocks), dim3(64), 0, st, A.B, A.P, A.pv, A.R, A.rec, A.adjm, (int64_t)0, S);
        } else {
            const int64_t blocks = (S + 255) / 256;
            hipLaunchKernelGGL(k_emit<kEmitRows>, dim3((unsigned)blocks), dim3(256), 0, st, A.B, A.P, A.pv, A.R, A.rec, A.adjm, (int64_t)0, S);
        }
    }
    // K3 (comfort mode, or any mode with draws): argmin + winner path
    if (!p.ref_direct) {
        const int64_t blocks = (S + kWinBlock - 1) / kWinBlock;
        if (A.wslot) {
            const unsigned b256 = (unsigned)((S + 255) / 256);
            hipLaunchKernelGGL((k_winner_st<false>), dim3(b256), dim3(256), 0, st, A.B, A.P, A.pv, A.R, (const double*)A.wslot);
            hipLaunchKernelGGL((k_winner_st<true>), dim3(b256), dim3(256), 0, st, A.B, A.P, A.pv, A.R, (const double*)A.wslot);
        } else {
            hipLaunchKernelGGL((k_winner<false>), dim3((unsigned)blocks), dim3(kWinBlock), 0, st, A.mg, A.B, A.P, A.pv, A.R);
            hipLaunchKernelGGL((k_winner<true>), dim3((unsigned)blocks), dim3(kWinBlock), 0, st, A.mg, A.B, A.P, A.pv, A.R);
        }
    }
    if (E.tall) (void)hipEventRecord(ev_at(E, 3), st);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    return PP_OK;
}

// pp_eval; fio (pp_plan_frame): the single-launch frame kernel with host-memory staging, where the
// call takes the fused one-launch shape (PP_ERR_STATE otherwise: the caller stages by copies)
int32_t eval_impl(pp_map* M, const pp_scene_batch* in, const pp_params* prm, pp_result* out,
                  int32_t device, void* hip_stream, const FrameIO* fio) {
    int32_t rc = eval_check(M, in, prm, out, device);
    if (rc || in->n_scenes == 0) return rc;
    DeviceGuard g(device);
    EvalPlan p;
    rc = eval_plan(M, in, prm, device, p);
    if (rc) return rc;
    if (fio && (!p.step_fused || p.groups_f != 1)) return PP_ERR_STATE;
    // the map lock is held from workspace binding through the (asynchronous) launches: a
    // concurrent call cannot grow and free this stream's buffers in between
    std::lock_guard<std::mutex> lk(M->mu);
    rc = dev_init(M, device);
    if (rc) return rc;
    DevState& DS = M->dev[device];
    StreamWS& W = DS.sws[hip_stream];
    EvalArgs A;
    rc = eval_bind(M, DS, W, in, prm, out, device, hip_stream, p, A);
    if (rc) return rc;
    if (dbg(PP_DBG_POISON)) {
        rc = poison_fill(W, A.st, p, prm, out);
        if (rc) return rc;
    }
    EvalEvents E = {&DS, DS.ev.rec.size(), DS.timing != 0, DS.timing == 1, DS.timing != 0};
    if (E.timing) {
        DS.ev.rec.resize(E.base + 4 * kPartMax, nullptr);
        // (bit 0: K4 is a kernel of its own, neither all paths nor inside the fused kernels)
        DS.ev.kind.push_back((!(p.ref_direct && prm->emit_paths) && !p.fused ? 1 : 0) | (E.tall ? 0 : 16));
    }
#ifdef PP_CHECK
    rc = check_limits(W, p, A);
    if (rc) return rc;
#endif
    A.persist = p.persist && !p.step_fused ? persist_blocks(DS, p.cg, device) : 0;
    g_dbg[PP_DBG_LAST_PERSIST].store((int)A.persist, std::memory_order_relaxed);
    A.persist_shape = A.persist && NL * kShapeSPB <= 64 && prm->n_speeds == kShapeNS && prm->n_points == 50 &&
                      p.cg.spb == kShapeSPB && p.cg.threads == 256;
    g_dbg[PP_DBG_LAST_PERSIST_SHAPE].store(A.persist_shape ? 1 : 0, std::memory_order_relaxed);
    if (p.step_fused) return launch_step(A, p, E, fio);
    // (the parts' flagged-group counts and, behind them, the persistent kernels' claim counters)
    if (hipMemsetAsync(A.gb.count, 0, (kPartMax + kPersistCtr) * sizeof(uint32_t), A.st) != hipSuccess) return PP_ERR_HIP;
    g_dbg[PP_DBG_LAST_PARTS].store(1, std::memory_order_relaxed);
    return p.split ? launch_split(A, p, E, W) : launch_plain(A, p, E);
}

}  // namespace
