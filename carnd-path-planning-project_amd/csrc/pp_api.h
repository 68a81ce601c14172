// pp_api.h — host: the C ABI (include/pp.h) except the rollouts and the host-memory frame path.
// Part of pp_eval.hip's translation unit.
#pragma once

extern "C" {

void pp_params_default(pp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->n_points = 50;
    p->n_speeds = 5;
    p->cost_mode = PP_COST_REFERENCE;
    p->emit_paths = 0;
    const double offs[4] = {-4.0, -2.0, 0.0, 2.0};      // SURVEY.md §8(d) speed grid
    for (int i = 0; i < 4; i++) p->speed_offsets[i] = offs[i];
    p->relaxed_acc = 5;                  // src/main.cpp:39-49
    p->min_relaxed_acc_while_braking = 4;
    p->maximum_acc = 8;
    p->max_speed = 22.2;
    p->car_length = 4.5;
    p->safety_distance = 2;
    p->keep_distance = 10;
    p->keep_distance_leeway = 0.5;
    p->n_draws = 0;
    p->noise_seed = 0x5EED0002ull;
    p->noise_first_scene = 0;
    p->noise_pos_sigma = 0.5;            // SURVEY.md §8(d) Monte-Carlo
    p->noise_vel_sigma = 0.5;
}

int32_t pp_num_candidates(const pp_params* p) { return p ? n_draws(p) * NL * p->n_speeds : 0; }

int32_t pp_num_lanes(void) { return NL; }

int32_t pp_max_cars(void) { return PP_MAX_CARS; }

double pp_mc_gauss(uint64_t seed, int64_t scene, int32_t draw, int32_t car, int32_t q) {
    return ppsynth::mc_gauss(seed, (uint64_t)scene, draw, car, q);
}

#ifdef PP_CHECK
int32_t pp_check_read(unsigned long long* out, int32_t reset) {  // checking builds only: g_chk[8]
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chk), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_chk), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef PP_TRACE
int32_t pp_trace_read(unsigned long long* out, int64_t words) {   // diagnostic builds only: g_trace
    if (words > 8LL * kTraceMax) words = 8LL * kTraceMax;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), sizeof(unsigned long long) * words) != hipSuccess) return -1;
    return 0;
}
#endif
#if defined(PP_DIAG) || defined(PP_LIMCENSUS)
int32_t pp_diag_read(unsigned long long* out, int32_t reset) {   // diagnostic builds only (96 words)
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), sizeof(unsigned long long) * kDiagWords) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[kDiagWords] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif
int32_t pp_libm_eval(int32_t kind, const double* a, const double* b, double* out, int64_t n,
                     int32_t device, void* hip_stream) {
    if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!a || !out || (kind == 2 && !b))) || device < -1 ||
        device >= kMaxDev)
        return PP_ERR_ARG;
    if (n == 0) return PP_OK;
    if (device < 0) {
        for (int64_t i = 0; i < n; i++) {
            double r = __builtin_nan("");
            if (kind == 0) ppg::sin(a[i], r);
            else if (kind == 1) ppg::cos(a[i], r);
            else r = ppg::atan2(a[i], b[i]);
            out[i] = r;
        }
        return PP_OK;
    }
    DeviceGuard g(device);
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return PP_ERR_ARG;
    hipLaunchKernelGGL(k_libm, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, kind, a, b, out, n);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

int32_t pp_math_eval(int32_t kind, const double* a, const double* b, const double* c, const double* d,
                     double* out0, double* out1, double* out2, int64_t n, int32_t device, void* hip_stream) {
    const MathArity ar = math_arity(kind);
    if (kind < 0 || kind >= PP_MATH_KINDS || ar.nin == 0 || n < 0 || device < 0 || device >= kMaxDev) return PP_ERR_ARG;
    const double* in[4] = {a, b, c, d};
    double* out[3] = {out0, out1, out2};
    for (int k = 0; k < ar.nin && n > 0; k++) if (!in[k]) return PP_ERR_ARG;
    for (int k = 0; k < ar.nout && n > 0; k++) if (!out[k]) return PP_ERR_ARG;
    if (n == 0) return PP_OK;
    DeviceGuard g(device);
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return PP_ERR_ARG;
    hipLaunchKernelGGL(k_math, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, kind, a, b, c, d,
                       out0, out1, out2, n);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

const char* pp_version(void) { return "pp-mi355x 0.1 (gfx950, fp64, lane-per-candidate)"; }

int32_t pp_map_create(const double* wx, const double* wy, int32_t n, pp_map** out) {
    if (!wx || !wy || !out || n < 3 || n > kMaxWaypoints) return PP_ERR_ARG;
    pp_map* M = new (std::nothrow) pp_map();
    if (!M) return PP_ERR_NOMEM;
    int rc;
    try { rc = build_map(M, wx, wy, n); } catch (...) { rc = PP_ERR_NOMEM; }   // (host allocations)
    if (rc != PP_OK) { delete M; return rc; }
    *out = M;
    return PP_OK;
}

// Map::Init on the device from device waypoint arrays; the derived tables are mirrored to the host
// (for pp_map_geometry, the host generator and other devices).
static int32_t map_create_device(const double* d_wx, const double* d_wy, int32_t n, int32_t device,
                                 void* hip_stream, pp_map** out) {
    if (!d_wx || !d_wy || !out || n < 3 || n > kMaxWaypoints || device < 0 || device >= kMaxDev) return PP_ERR_ARG;
    DeviceGuard g(device);        // (declared first: the owners below are released on this device)
    std::unique_ptr<pp_map> M(new (std::nothrow) pp_map());
    if (!M) return PP_ERR_NOMEM;
    M->n = n;
    hipStream_t st = (hipStream_t)hip_stream;
    DevTables T;
    DevMem<int> bad;
    if (T.map.alloc(kMapArrays * (size_t)n) != PP_OK || T.lanetab.alloc(5 * NL * (size_t)n) != PP_OK ||
        bad.alloc(1) != PP_OK)
        return PP_ERR_NOMEM;
    // from here on the map kernels may be in flight: every exit, an exception's included, drains
    // `st` before the buffers above are released (declared after them, so it runs first)
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
    int rc = PP_OK;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (hipMemsetAsync(bad.get(), 0, sizeof(int), st) != hipSuccess) rc = PP_ERR_HIP;
    hipLaunchKernelGGL(k_map_normals, dim3(blocks), dim3(256), 0, st, d_wx, d_wy, n, T.map.get(), bad.get());
    hipLaunchKernelGGL(k_map_lanes, dim3(blocks), dim3(256), 0, st, n, T.map.get());
    hipLaunchKernelGGL(k_map_lengths, dim3(blocks), dim3(256), 0, st, n, T.map.get(), T.lanetab.get());
    if (hipGetLastError() != hipSuccess) rc = PP_ERR_HIP;
    int hbad = 0;
    M->geom.assign(kMapArrays * (size_t)n, 0.0);
    M->lanetab.assign(5 * NL * (size_t)n, 0.0);
    if (rc == PP_OK && (hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipMemcpyAsync(M->geom.data(), T.map.get(), sizeof(double) * kMapArrays * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipMemcpyAsync(M->lanetab.data(), T.lanetab.get(), sizeof(double) * 5 * NL * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess))
        rc = PP_ERR_HIP;
    if (rc == PP_OK && hbad) rc = PP_ERR_ARG;          // Map::Init divides by a zero segment length
    if (rc != PP_OK) return rc;
    fill_ptab(M.get());
    build_tables(M.get());
    fill_arctab(M.get());
    if (upload_wgrid(M.get(), T) != PP_OK) return PP_ERR_NOMEM;
    M->dev[device].tab = std::move(T);
    M->dev[device].init = true;
    *out = M.release();
    return PP_OK;
}
int32_t pp_map_create_device(const double* d_wx, const double* d_wy, int32_t n, int32_t device, void* hip_stream,
                             pp_map** out) {
    try { return map_create_device(d_wx, d_wy, n, device, hip_stream, out); } catch (...) { return PP_ERR_NOMEM; }   // (host allocations)
}

// every device the runtime has, initialised for this map or not, in turn: made current, drained,
// and its state released while it is current (the owners' destructors, which may run with another
// device current, then find nothing left to do)
int32_t pp_map_destroy(pp_map* M) {
    if (!M) return PP_ERR_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess) nd = 0;
    for (int d = 0; d < nd && d < kMaxDev; d++) {
        DeviceGuard g(d);
        (void)hipDeviceSynchronize();
        static_cast<DevRes&>(M->dev[d]) = DevRes();
    }
    delete M;
    return PP_OK;
}

int32_t pp_map_geometry(const pp_map* M, double* out, int32_t n) {
    if (!M || !out || n != M->n) return PP_ERR_ARG;
    memcpy(out, M->ptab.data(), sizeof(double) * (4 + 2 * NL) * (size_t)n);
    return PP_OK;
}

int32_t pp_reserve(pp_map* M, int32_t device, int64_t max_scenes) {
    if (!M || device < 0 || device >= kMaxDev || max_scenes < 0) return PP_ERR_ARG;
    std::lock_guard<std::mutex> lk(M->mu);
    DeviceGuard g(device);
    int rc = dev_init(M, device);
    if (rc) return rc;
    StreamWS& W = M->dev[device].sws[nullptr];       // the null stream's workspace
    rc = ensure_ws(W, nullptr, max_scenes);
    return rc ? rc : ensure_rec(W, nullptr, max_scenes);
}

int32_t pp_eval(pp_map* M, const pp_scene_batch* in, const pp_params* prm, pp_result* out,
                int32_t device, void* hip_stream) {
    return eval_impl(M, in, prm, out, device, hip_stream, nullptr);
}

int32_t pp_debug_set(int32_t key, int32_t value) {
    bool ok = false;
    switch (key) {
        case PP_DBG_PREP_GROUP: ok = prep_group_ok(value); break;
        case PP_DBG_PREP_WAVES: ok = value == 0 || value == 3 || value == 4; break;
        case PP_DBG_SHAPE: ok = value >= 0 && value <= PP_SHAPE_STEP; break;
        case PP_DBG_POISON: ok = value == 0 || value == 1; break;
        case PP_DBG_SPLIT: ok = value >= 0 && value <= 2; break;
        case PP_DBG_SORT_CARS: ok = value >= 0 && value <= 2; break;
        case PP_DBG_PERSIST: ok = value >= 0 && value <= 2; break;
        default: break;       // (PP_DBG_LAST_PARTS, PP_DBG_LAST_PERSIST and PP_DBG_LAST_PERSIST_SHAPE are read-only)
    }
    if (!ok) return PP_ERR_ARG;
    g_dbg[key].store(value, std::memory_order_relaxed);
    return PP_OK;
}

int32_t pp_debug_get(int32_t key) { return key >= 0 && key < PP_DBG_KEYS ? dbg(key) : PP_ERR_ARG; }

int32_t pp_timing_enable(pp_map* M, int32_t device, int32_t enable) {
    if (!M || device < 0 || device >= kMaxDev) return PP_ERR_ARG;
    std::lock_guard<std::mutex> lk(M->mu);
    DevState& D = M->dev[device];
    D.timing = enable == PP_TIMING_K2 ? 2 : (enable != 0 ? 1 : 0);
    if (D.timing) {
        // events made now, outside any timed region: 2,048 calls of K2-only timing (2 events each,
        // 2 per part when split) or 1,024 of all-kernel timing (4 per part); pp_eval takes the
        // events it records from this pool, pp_timing_read returns them
        DeviceGuard g(device);
        const int rc = dev_init(M, device);
        if (rc) return rc;
        while (D.ev.pool.size() + D.ev.rec.size() < 4 * kSplitMax * 256) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return PP_ERR_HIP;
            D.ev.pool.push_back(e);
        }
    }
    return PP_OK;
}

int32_t pp_timing_read(pp_map* M, int32_t device, double* ms3, int64_t* launches3) {
    if (!M || device < 0 || device >= kMaxDev || !ms3 || !launches3) return PP_ERR_ARG;
    std::lock_guard<std::mutex> lk(M->mu);
    DevState& D = M->dev[device];
    DeviceGuard g(device);
    for (int k = 0; k < 3; k++) { ms3[k] = 0; launches3[k] = 0; }
    int rc = PP_OK;
    constexpr int EG = 4 * kPartMax;
    const size_t ng = D.ev.rec.size() / EG;
    // signed milliseconds from a to b (either order)
    auto dt = [&](hipEvent_t a, hipEvent_t b, float& t) {
        if (!a || !b) { rc = PP_ERR_HIP; return false; }
        if (hipEventElapsedTime(&t, a, b) == hipSuccess) return true;
        if (hipEventElapsedTime(&t, b, a) == hipSuccess) { t = -t; return true; }
        rc = PP_ERR_HIP;
        return false;
    };
    for (size_t i = 0; i < ng; i++) {
        const int kind = D.ev.kind[i], parts = (kind >> 8) & 0xFF, np = parts ? parts : 1;
        const int per = (kind >> 16) & 0xF, pc = per ? per : np;    // parts per chunk
        const bool k2only = (kind & 16) != 0;
        hipEvent_t* e0 = &D.ev.rec[EG * i];
        for (int h = 0; h < np; h++) {
            hipEvent_t last = k2only ? e0[4 * h + 2] : e0[4 * h + 3];
            if (!last || hipEventSynchronize(last) != hipSuccess) rc = PP_ERR_HIP;
        }
        // stage k (0: K1, 1: K2, 2: K3/K4) of a call: per chunk, from its earliest start to its
        // latest end over the chunk's parts (one stream: the kernel's own interval; a split call's
        // parts overlap, and the stage's time is the span they cover together, as in a kernel
        // trace), summed over the chunks; one launch per call
        for (int k = 0; k < 3; k++) {
            if (k != 1 && (k2only || (k == 0 && (kind & 32)) || (k == 2 && !(kind & 1)))) continue;
            float sum = 0;
            bool ok = true;
            for (int c0 = 0; c0 < np && ok; c0 += pc) {
                float lo = 0, hi = 0;
                for (int h = c0; h < std::min(np, c0 + pc) && ok; h++) {
                    float a, b;
                    ok = dt(e0[1], e0[4 * h + k], a) && dt(e0[1], e0[4 * h + k + 1], b);
                    if (ok) { lo = h == c0 ? a : std::min(lo, a); hi = h == c0 ? b : std::max(hi, b); }
                }
                sum += hi - lo;
            }
            if (ok) { ms3[k] += sum; launches3[k]++; }
        }
        for (int k = 0; k < EG; k++)
            if (e0[k]) D.ev.pool.push_back(e0[k]);
    }
    D.ev.rec.clear();
    D.ev.kind.clear();
    return rc;
}

int32_t pp_synth_scenes(pp_map* M, uint64_t seed, int64_t first_scene, pp_scene_batch* out,
                        int32_t device, void* hip_stream) {
    if (!M || !out || device < 0 || device >= kMaxDev || out->n_scenes < 0 || first_scene < 0) return PP_ERR_ARG;
    if (out->car_stride < ppsynth::kSynthCars) return PP_ERR_ARG;
    if (out->n_scenes == 0) return PP_OK;
    const WorldDev W(M, device, false);
    if (W.rc) return W.rc;
    const ppsynth::OutBatch o = out_batch(out);
    return launch_scenes(k_synth, o.S, hip_stream, W.T, seed, first_scene, o);
}

int32_t pp_synth_scenes_host(const pp_map* M, uint64_t seed, int64_t first_scene, pp_scene_batch* out) {
    if (!M || !out || out->n_scenes < 0 || first_scene < 0 || out->car_stride < ppsynth::kSynthCars) return PP_ERR_ARG;
    const ppsynth::LaneTables T = host_tables(M).T;
    const ppsynth::OutBatch o = out_batch(out);
    for (int64_t s = 0; s < o.S; s++) ppsynth::synth_scene(T, seed, first_scene + s, s, o);
    return PP_OK;
}

int32_t pp_synth_traffic(pp_map* M, uint64_t seed, int64_t first_scene, pp_scene_batch* tel,
                         pp_traffic* out, int32_t device, void* hip_stream) {
    if (!M || !tel || device < 0 || device >= kMaxDev || tel->n_scenes < 0 || first_scene < 0 ||
        tel->car_stride < ppsynth::kSynthCars || !traffic_ok(out, tel) ||
        (tel->tab_valid && (tel->tab_slots < ppsynth::kSynthCars || tel->tab_slots > PP_MAX_CARS)))
        return PP_ERR_ARG;
    if (tel->n_scenes == 0) return PP_OK;
    const WorldDev W(M, device, false);
    if (W.rc) return W.rc;
    out->n_cars = ppsynth::kSynthCars;
    const ppsynth::OutBatch o = out_batch(tel);
    return launch_scenes(k_synth_traffic, o.S, hip_stream, W.T, seed, first_scene, o, traffic_view(out, o.S), *tel);
}

int32_t pp_synth_traffic_host(const pp_map* M, uint64_t seed, int64_t first_scene, pp_scene_batch* tel,
                              pp_traffic* out) {
    if (!M || !tel || tel->n_scenes < 0 || first_scene < 0 || tel->car_stride < ppsynth::kSynthCars ||
        !traffic_ok(out, tel) ||
        (tel->tab_valid && (tel->tab_slots < ppsynth::kSynthCars || tel->tab_slots > PP_MAX_CARS)))
        return PP_ERR_ARG;
    const ppsynth::LaneTables T = host_tables(M).T;
    out->n_cars = ppsynth::kSynthCars;
    const ppsynth::OutBatch o = out_batch(tel);
    const ppsynth::TrafficV tv = traffic_view(out, o.S);
    for (int64_t s = 0; s < o.S; s++) {
        ppsynth::synth_scene(T, seed, first_scene + s, s, o, &tv);
        for (int j = 0; tel->tab_valid && j < tel->tab_slots; j++) {
            tel->tab_valid[(int64_t)j * o.S + s] = 0;
            if (tel->tab_id) tel->tab_id[(int64_t)j * o.S + s] = j;
        }
    }
    return PP_OK;
}

}  // extern "C"
