// pp_api_frame.h — host: pp_plan_batch_host, pp_plan_reset, pp_plan_frame (C ABI).
// Part of pp_eval.hip's translation unit.
#pragma once

extern "C" {

// Host-memory batch (the batched onMessage): stage the scenes (and their car table) into device
// memory, pp_eval, copy results (and the updated table) back. Synchronous.
// pp_plan_batch_host stages batches up to this many scenes through its pinned mirror
constexpr int64_t kStageMirrorMax = 512;
int32_t pp_plan_batch_host(pp_map* M, int32_t device, pp_scene_batch* hin, const pp_params* prm,
                           pp_result* hout, void* hip_stream) {
    if (!M || !hin || !prm || !hout || device < 0 || device >= kMaxDev || !params_ok(prm) || prm->emit_paths ||
        hin->n_scenes < 0 || hin->car_stride < 0 || hin->car_stride > PP_MAX_CARS)
        return PP_ERR_ARG;
    if (!hout->winner || !hout->n_out || !hout->next_x || !hout->next_y || !hout->cost || !hout->status)
        return PP_ERR_ARG;
    const int64_t S = hin->n_scenes;
    if (S == 0) return PP_OK;
    const int J = hin->car_stride, N = prm->n_points;
    const int C = n_draws(prm) * NL * prm->n_speeds;
    const bool tab = hin->tab_valid != nullptr;
    // staging layout: doubles first, then 4-byte fields
    const int TS = tab ? hin->tab_slots : 0;
    if (tab && (TS < 0 || TS > PP_MAX_CARS)) return PP_ERR_ARG;
    // every host pointer the staging copies touch (small batches memcpy them on the host, so a
    // NULL here must be refused before staging, not left to the copy)
    if (!hin->ego_x || !hin->ego_y || !hin->ego_yaw_deg || !hin->ego_speed_mph || !hin->prev_x || !hin->prev_y ||
        !hin->n_prev || !hin->prev_target_lane || !hin->n_cars)
        return PP_ERR_ARG;
    if (J > 0 && (!hin->car_id || !hin->car_x || !hin->car_y || !hin->car_vx || !hin->car_vy)) return PP_ERR_ARG;
    if (tab && TS > 0 && (!hin->tab_lane || !hin->tab_s || !hin->tab_d || !hin->tab_vs || !hin->tab_vd ||
                          !hin->tab_vx || !hin->tab_vy))
        return PP_ERR_ARG;
    const size_t nd = (size_t)S * (4 + 2 * PP_PREV_KEEP + 4 * J + 6 * TS + 2 * N + C);
    const size_t ni = (size_t)S * (3 + J + 3 * TS + 3);
    const size_t bytes = nd * 8 + ni * 4 + 256;
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)hip_stream;
    std::lock_guard<std::mutex> stage_lock(M->dev[device].stage_mu);
    char* base;
    char* mirror;                 // pinned host mirror of the staging buffer (same offsets)
    {
        std::lock_guard<std::mutex> lk(M->mu);
        int rc = dev_init(M, device);
        if (rc) return rc;
        DevState& D = M->dev[device];
        if (D.stage.cap() < (int64_t)bytes) {
            // the old pair goes first, once the device has drained (earlier calls may have staged
            // on any stream); the new buffers are kept only as a pair
            if (D.stage) (void)hipDeviceSynchronize();
            D.stage.reset(); D.stage_host.reset();
            DevMem<> dev;
            Pinned host;
            rc = dev.grow(st, (int64_t)bytes, bytes);
            if (!rc) rc = host.alloc(bytes, hipHostMallocDefault);
            if (rc) return rc;
            D.stage = std::move(dev); D.stage_host = std::move(host);
        }
        base = (char*)D.stage.get();
        mirror = (char*)D.stage_host.get();
    }
    double* dp = (double*)base;
    int32_t* ip = (int32_t*)(base + nd * 8);
    auto takeD = [&](size_t n) { double* r = dp; dp += n; return r; };
    auto takeI = [&](size_t n) { int32_t* r = ip; ip += n; return r; };
    bool ok = true;
    // Small batches (latency): inputs are gathered into the pinned mirror; the input fields lead
    // each region (doubles, then ints), so one copy per region moves them, and one per region
    // brings the outputs back. Large batches (bandwidth): one asynchronous copy per field straight
    // from and to the caller's buffers (the extra host memcpy through the mirror costs more there).
    const bool small = S <= kStageMirrorMax;
    auto h2d = [&](void* d, const void* h, size_t n) {
        if (!n) return;
        if (small) memcpy(mirror + ((char*)d - base), h, n);
        else if (hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st) != hipSuccess) ok = false;
    };
    pp_scene_batch B;
    memset(&B, 0, sizeof(B));
    B.n_scenes = S; B.car_stride = J;
    double* ego = takeD(4 * S);
    B.ego_x = ego; B.ego_y = ego + S; B.ego_yaw_deg = ego + 2 * S; B.ego_speed_mph = ego + 3 * S;
    h2d(ego, hin->ego_x, 8 * S); h2d(ego + S, hin->ego_y, 8 * S);
    h2d(ego + 2 * S, hin->ego_yaw_deg, 8 * S); h2d(ego + 3 * S, hin->ego_speed_mph, 8 * S);
    double* pxy = takeD(2 * PP_PREV_KEEP * S);
    B.prev_x = pxy; B.prev_y = pxy + PP_PREV_KEEP * S;
    h2d(pxy, hin->prev_x, 8 * PP_PREV_KEEP * S); h2d(pxy + PP_PREV_KEEP * S, hin->prev_y, 8 * PP_PREV_KEEP * S);
    double* cars = takeD(4 * (size_t)J * S);
    B.car_x = cars; B.car_y = cars + J * S; B.car_vx = cars + 2 * J * S; B.car_vy = cars + 3 * J * S;
    if (J) {
        h2d(cars, hin->car_x, 8 * J * S); h2d(cars + J * S, hin->car_y, 8 * J * S);
        h2d(cars + 2 * J * S, hin->car_vx, 8 * J * S); h2d(cars + 3 * J * S, hin->car_vy, 8 * J * S);
    }
    double* tabd = nullptr;
    if (tab) {
        tabd = takeD(6 * (size_t)TS * S);
        const double* src[6] = {hin->tab_s, hin->tab_d, hin->tab_vs, hin->tab_vd, hin->tab_vx, hin->tab_vy};
        double** dst[6] = {&B.tab_s, &B.tab_d, &B.tab_vs, &B.tab_vd, &B.tab_vx, &B.tab_vy};
        for (int k = 0; k < 6; k++) { *dst[k] = tabd + k * (size_t)TS * S; h2d(*dst[k], src[k], 8 * (size_t)TS * S); }
        B.tab_slots = TS;
    }
    double* nxy = takeD(2 * (size_t)N * S);
    double* cost = takeD((size_t)C * S);
    int32_t* ints = takeI(3 * S);
    B.n_prev = ints; B.prev_target_lane = ints + S; B.n_cars = ints + 2 * S;
    h2d(ints, hin->n_prev, 4 * S); h2d(ints + S, hin->prev_target_lane, 4 * S); h2d(ints + 2 * S, hin->n_cars, 4 * S);
    int32_t* cid = takeI((size_t)J * S);
    B.car_id = cid;
    h2d(cid, hin->car_id, 4 * J * S);
    int32_t* tabi = nullptr;
    if (tab) {
        tabi = takeI(3 * (size_t)TS * S);
        B.tab_valid = tabi; B.tab_lane = tabi + (size_t)TS * S;
        h2d(tabi, hin->tab_valid, 4 * (size_t)TS * S); h2d(tabi + (size_t)TS * S, hin->tab_lane, 4 * (size_t)TS * S);
        if (hin->tab_id) { B.tab_id = tabi + 2 * (size_t)TS * S; h2d(B.tab_id, hin->tab_id, 4 * (size_t)TS * S); }
    }
    int32_t* outi = takeI(3 * S);
    pp_result R;
    memset(&R, 0, sizeof(R));
    R.winner = outi; R.n_out = outi + S; R.status = (uint32_t*)(outi + 2 * S);
    R.next_x = nxy; R.next_y = nxy + (size_t)N * S; R.cost = cost;
    const char* d_in_end = (const char*)nxy;           // doubles: inputs [base, nxy)
    const char* i_beg = base + nd * 8;                  // ints: inputs [i_beg, outi)
    const char* d_out_beg = tab ? (const char*)tabd : (const char*)nxy;   // outputs: (tables,) plans, costs
    const char* d_out_end = (const char*)(cost + (size_t)C * S);
    const char* i_out_beg = tab ? (const char*)tabi : (const char*)outi;
    const char* i_out_end = (const char*)(outi + 3 * S);
    auto copy = [&](const char* lo, const char* hi, bool in) {
        if (hi <= lo) return;
        char* h = mirror + (lo - base);
        if (hipMemcpyAsync(in ? (void*)lo : (void*)h, in ? (const void*)h : (const void*)lo, (size_t)(hi - lo),
                           in ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st) != hipSuccess) ok = false;
    };
    if (small) { copy(base, d_in_end, true); copy(i_beg, (const char*)outi, true); }
    if (!ok) return PP_ERR_HIP;
    int rc = pp_eval(M, &B, prm, &R, device, hip_stream);
    if (rc != PP_OK) return rc;
    if (small && dbg(PP_DBG_POISON)) {   // the mirror's pure-output regions (inputs may still be in flight)
        memset(mirror + ((const char*)nxy - base), 0xFF, (size_t)(d_out_end - (const char*)nxy));
        memset(mirror + ((const char*)outi - base), 0xFF, (size_t)(i_out_end - (const char*)outi));
    }
    if (small) {
        copy(d_out_beg, d_out_end, false);
        copy(i_out_beg, i_out_end, false);
        if (!ok || hipStreamSynchronize(st) != hipSuccess) return PP_ERR_HIP;
    }
    auto d2h = [&](void* h, const void* d, size_t n) {
        if (!n) return;
        if (small) memcpy(h, mirror + ((const char*)d - base), n);
        else if (hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st) != hipSuccess) ok = false;
    };
    d2h(hout->winner, R.winner, 4 * S); d2h(hout->n_out, R.n_out, 4 * S); d2h(hout->status, R.status, 4 * S);
    d2h(hout->next_x, R.next_x, 8 * (size_t)N * S); d2h(hout->next_y, R.next_y, 8 * (size_t)N * S);
    d2h(hout->cost, R.cost, 8 * (size_t)C * S);
    if (tab) {
        double* dstd[6] = {hin->tab_s, hin->tab_d, hin->tab_vs, hin->tab_vd, hin->tab_vx, hin->tab_vy};
        for (int k = 0; k < 6; k++) d2h(dstd[k], tabd + k * (size_t)TS * S, 8 * (size_t)TS * S);
        d2h(hin->tab_valid, tabi, 4 * (size_t)TS * S); d2h(hin->tab_lane, tabi + (size_t)TS * S, 4 * (size_t)TS * S);
    }
    if (!small && (!ok || hipStreamSynchronize(st) != hipSuccess)) return PP_ERR_HIP;
    return PP_OK;
}

int32_t pp_plan_reset(pp_map* M, int32_t device) {
    if (!M || device < 0 || device >= kMaxDev) return PP_ERR_ARG;
    std::lock_guard<std::mutex> lk(M->dev[device].frame_mu);
    M->dev[device].plan_table.cars.clear();
    return PP_OK;
}

// One telemetry frame (the onMessage replacement): C = 3 (one speed: max_speed), reference mode.
#ifdef PP_FRAME_PROF
// diagnostic builds (-DPP_FRAME_PROF): per-frame host and device intervals, summed (us) — host:
// staging until the launch, the launch call, launch-to-done, done-to-return; device (100 MHz
// clock): input copy, the frame's body, output copy; and the frame count. pp_frame_prof_read
// returns and clears them.
static double g_fprof[8];
static double fprof_now() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int32_t pp_frame_prof_read(double* out8) {
    for (int i = 0; i < 8; i++) { out8[i] = g_fprof[i]; g_fprof[i] = 0; }
    return PP_OK;
}
#endif
int32_t pp_plan_frame(pp_map* M, int32_t device, double ego_x, double ego_y, double ego_yaw_deg,
                      double ego_speed_mph, const double* prev_x, const double* prev_y, int32_t n_prev,
                      const int32_t* car_id, const double* car_x, const double* car_y,
                      const double* car_vx, const double* car_vy, int32_t n_cars,
                      int32_t* target_lane, double* next_x, double* next_y, int32_t* n_out) {
    if (!M || !target_lane || !next_x || !next_y || !n_out || n_cars < 0 || n_cars > PP_MAX_CARS ||
        device < 0 || device >= kMaxDev || (n_prev > 0 && (!prev_x || !prev_y)) ||
        (n_cars > 0 && (!car_id || !car_x || !car_y || !car_vx || !car_vy)))
        return PP_ERR_ARG;
    if (*target_lane < 0 || *target_lane >= NL) return PP_ERR_ARG;
#ifdef PP_FRAME_PROF
    const double h0 = fprof_now();
#endif
    // host staging: one scene, SoA with S = 1 (std::map order: stable sort by id, last row of a
    // duplicated id wins as in `sensor_fusion_cars[id]` assignment, src/main.cpp:1329)
    struct Row { int32_t id; double x, y, vx, vy; };
    std::vector<Row> rows;
    for (int j = 0; j < n_cars; j++) {
        bool dup = false;
        for (auto& r : rows) if (r.id == car_id[j]) { r = {car_id[j], car_x[j], car_y[j], car_vx[j], car_vy[j]}; dup = true; }
        if (!dup) rows.push_back({car_id[j], car_x[j], car_y[j], car_vx[j], car_vy[j]});
    }
    std::stable_sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.id < b.id; });
    const int nc = (int)rows.size();
    // device scratch layout (bytes): doubles then ints, then the scene info (the target lane)
    constexpr int N = 50;
    constexpr int TS = PP_MAX_CARS;
    struct Frame {
        double ego[4], px[PP_PREV_KEEP], py[PP_PREV_KEEP], cx[PP_MAX_CARS], cy[PP_MAX_CARS],
            cvx[PP_MAX_CARS], cvy[PP_MAX_CARS];
        double nx[N], ny[N], cost[NL];
        double ts[TS], td[TS], tvs[TS], tvd[TS], tvx[TS], tvy[TS];        // the car table's slots
        int32_t tid[TS], tvalid[TS], tlane[TS];
        int32_t nprev, ptl, ncars, cid[PP_MAX_CARS], winner, nout;
        uint32_t status;
        pp_scene_info info;
    };
    DeviceGuard g(device);
    std::lock_guard<std::mutex> frame_lock(M->dev[device].frame_mu);
    DevState& DS = M->dev[device];
    Frame* d = nullptr;
    constexpr size_t kFlagOff = (sizeof(Frame) + 63) / 64 * 64;
    {   // per-device scratch, made once: the device frame, its pinned host copy, the frame stream
        std::lock_guard<std::mutex> lk(M->mu);
        int rc = dev_init(M, device);
        if (rc) return rc;
        // (both copies kFlagOff bytes: the 16-B units of the last fields may pass sizeof(Frame))
        if (DS.frame.grow(nullptr, 1, kFlagOff) != PP_OK) return PP_ERR_NOMEM;
        if (!DS.frame_host) {
            if (DS.frame_host.alloc(kFlagOff + 64, hipHostMallocMapped | hipHostMallocCoherent) != PP_OK)
                return PP_ERR_NOMEM;
            memset(DS.frame_host.get(), 0, kFlagOff + 64);
            DS.frame_seq = 0;
        }
        if (!DS.frame_stream && hipStreamCreateWithFlags(DS.frame_stream.out(), hipStreamNonBlocking) != hipSuccess)
            return PP_ERR_HIP;
        d = (Frame*)DS.frame.get();
    }
    Frame& h = *(Frame*)DS.frame_host.get();
    volatile uint32_t* flag = (volatile uint32_t*)((char*)DS.frame_host.get() + kFlagOff);
    // (only the words the frame's ranges carry are written: the previous path's unused tail is
    // zeroed, every other input range is filled below)
    memset(h.px, 0, sizeof h.px); memset(h.py, 0, sizeof h.py);
    const bool poison = dbg(PP_DBG_POISON) != 0;
    if (poison) {     // the outputs' staging starts NaN-filled (pp_eval poisons them on the device too)
        memset(h.nx, 0xFF, sizeof h.nx); memset(h.ny, 0xFF, sizeof h.ny); memset(h.cost, 0xFF, sizeof h.cost);
        memset(&h.winner, 0xFF, sizeof h.winner); memset(&h.nout, 0xFF, sizeof h.nout);
        memset(&h.status, 0xFF, sizeof h.status); memset(&h.info, 0xFF, sizeof h.info);
    }
    h.ego[0] = ego_x; h.ego[1] = ego_y; h.ego[2] = ego_yaw_deg; h.ego[3] = ego_speed_mph;
    for (int i = 0; i < PP_PREV_KEEP && i < n_prev; i++) { h.px[i] = prev_x[i]; h.py[i] = prev_y[i]; }
    h.nprev = n_prev; h.ptl = *target_lane; h.ncars = nc;
    for (int j = 0; j < nc; j++) {
        h.cid[j] = rows[j].id; h.cx[j] = rows[j].x; h.cy[j] = rows[j].y; h.cvx[j] = rows[j].vx; h.cvy[j] = rows[j].vy;
    }
    // the reference's std::map, laid out over the union of its ids and this frame's (any ints)
    const pptab::Slots hs = {1, h.tid, h.tvalid, h.tlane, h.ts, h.td, h.tvs, h.tvd, h.tvx, h.tvy};
    const int nu = DS.plan_table.union_size(h.cid, nc);
    if (nu > TS) return PP_ERR_ARG;                     // more than PP_MAX_CARS distinct cars
    const int nslots = DS.plan_table.layout(h.cid, nc, hs, 0, nu, poison);
    if (nslots < 0) return PP_ERR_ARG;
    hipStream_t st = DS.frame_stream.get();
    pp_scene_batch B;
    memset(&B, 0, sizeof(B));
    B.n_scenes = 1; B.car_stride = PP_MAX_CARS;
    B.ego_x = &d->ego[0]; B.ego_y = &d->ego[1]; B.ego_yaw_deg = &d->ego[2]; B.ego_speed_mph = &d->ego[3];
    B.prev_x = d->px; B.prev_y = d->py; B.n_prev = &d->nprev; B.prev_target_lane = &d->ptl;
    B.n_cars = &d->ncars; B.car_id = d->cid; B.car_x = d->cx; B.car_y = d->cy; B.car_vx = d->cvx; B.car_vy = d->cvy;
    B.tab_slots = nslots; B.tab_id = d->tid;
    B.tab_valid = d->tvalid; B.tab_lane = d->tlane; B.tab_s = d->ts; B.tab_d = d->td;
    B.tab_vs = d->tvs; B.tab_vd = d->tvd; B.tab_vx = d->tvx; B.tab_vy = d->tvy;
    pp_params P;
    pp_params_default(&P);
    P.n_speeds = 1;
    pp_result R;
    memset(&R, 0, sizeof(R));
    R.winner = &d->winner; R.n_out = &d->nout; R.next_x = d->nx; R.next_y = d->ny; R.cost = d->cost;
    R.status = &d->status; R.info = &d->info;
    // The frame's words that carry data: inputs (ego, previous path, this frame's rows, the table's
    // nslots slots) and outputs (plan, costs, winner / count / status / info, the slots again).
    FrameIO io;
    memset(&io, 0, offsetof(FrameIO, inl));
    // (each field's bytes rounded out to whole 16-B units: the extra words are other fields of the
    // frame — inputs the kernel overwrites nothing of, outputs the host does not read — and a unit
    // range touching the previous one joins it)
    bool fio_full = false;        // a range beyond the kernel argument's kFioMax (never: 15 in, 10 out)
    auto add = [&](bool in, const void* p, size_t bytes) {
        if (!bytes) return;
        const size_t b0 = (size_t)((const char*)p - (const char*)&h);
        const uint32_t u0 = (uint32_t)(b0 / 16), u1 = (uint32_t)((b0 + bytes + 15) / 16);
        int& n = in ? io.n_in : io.n_out;
        uint32_t* off = in ? io.in_off : io.out_off;
        uint32_t* len = in ? io.in_len : io.out_len;
        if (n > 0 && u0 <= off[n - 1] + len[n - 1] && u0 >= off[n - 1]) {
            if (u1 > off[n - 1] + len[n - 1]) len[n - 1] = u1 - off[n - 1];
            return;
        }
        if (n >= kFioMax) { fio_full = true; return; }
        off[n] = u0; len[n] = u1 - u0;
        n++;
    };
    const size_t ns = (size_t)nslots, ncs = (size_t)nc;
    add(true, h.ego, sizeof h.ego + sizeof h.px + sizeof h.py);   // ego, px, py: adjacent
    add(true, h.cx, 8 * ncs); add(true, h.cy, 8 * ncs); add(true, h.cvx, 8 * ncs); add(true, h.cvy, 8 * ncs);
    add(true, h.ts, 8 * ns); add(true, h.td, 8 * ns); add(true, h.tvs, 8 * ns); add(true, h.tvd, 8 * ns);
    add(true, h.tvx, 8 * ns); add(true, h.tvy, 8 * ns);
    add(true, h.tid, 4 * ns); add(true, h.tvalid, 4 * ns); add(true, h.tlane, 4 * ns);
    add(true, &h.nprev, 4 * (3 + ncs));                          // nprev, ptl, ncars, cid[nc]: adjacent
    add(false, h.nx, sizeof h.nx + sizeof h.ny + sizeof h.cost);  // nx, ny, cost: adjacent
    add(false, h.ts, 8 * ns); add(false, h.td, 8 * ns); add(false, h.tvs, 8 * ns); add(false, h.tvd, 8 * ns);
    add(false, h.tvx, 8 * ns); add(false, h.tvy, 8 * ns);
    add(false, h.tvalid, 4 * ns); add(false, h.tlane, 4 * ns);
    add(false, &h.winner, (size_t)((const char*)(&h.info + 1) - (const char*)&h.winner));   // winner .. info
    static_assert(offsetof(Frame, px) == offsetof(Frame, ego) + sizeof(double) * 4 &&
                  offsetof(Frame, py) == offsetof(Frame, px) + sizeof(double) * PP_PREV_KEEP &&
                  offsetof(Frame, ny) == offsetof(Frame, nx) + sizeof(double) * N &&
                  offsetof(Frame, cost) == offsetof(Frame, ny) + sizeof(double) * N &&
                  offsetof(Frame, cid) == offsetof(Frame, nprev) + 12 && sizeof(pp_scene_info) % 4 == 0,
                  "adjacent frame fields");
    if (fio_full) return PP_ERR_STATE;
    {   // the input units in range order, inline where they fit
        int nu = 0;
        for (int r = 0; r < io.n_in; r++) nu += (int)io.in_len[r];
        io.n_inl = 0;
        if (nu <= kFioInline) {
            const uint4* hu = (const uint4*)&h;
            for (int r = 0; r < io.n_in; r++)
                for (uint32_t w = 0; w < io.in_len[r]; w++) io.inl[io.n_inl++] = hu[io.in_off[r] + w];
        }
    }
    void* hdev = nullptr;
    if (hipHostGetDevicePointer(&hdev, DS.frame_host.get(), 0) != hipSuccess) return PP_ERR_HIP;
    io.h_in = (const uint4*)hdev; io.h_out = (uint4*)hdev; io.d_frame = (uint4*)d;
    io.h_flag = (uint32_t*)((char*)hdev + kFlagOff);
    io.seq = ++DS.frame_seq;
#ifdef PP_FRAME_PROF
    const double h1 = fprof_now();
#endif
    int rc = eval_impl(M, &B, &P, &R, device, (void*)st, &io);
#ifdef PP_FRAME_PROF
    const double h2 = fprof_now();
#endif
    if (rc == PP_OK) {
        // the kernel's done word; the stream is polled now and then, so a failed launch or a fault
        // ends the wait with an error
        for (uint64_t spin = 1; *flag != io.seq; spin++) {
            if ((spin & 1023) == 0) {
                const hipError_t e = hipStreamQuery(st);
                if (e == hipSuccess && *flag != io.seq) { rc = PP_ERR_HIP; break; }
                if (e != hipSuccess && e != hipErrorNotReady) { rc = PP_ERR_HIP; break; }
            }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        std::atomic_thread_fence(std::memory_order_acquire);
#ifdef PP_FRAME_PROF
        const double h3 = fprof_now();
        const volatile uint32_t* fw = flag;
        g_fprof[0] += h1 - h0; g_fprof[1] += h2 - h1; g_fprof[2] += h3 - h2;
        g_fprof[4] += (uint32_t)(fw[5] - fw[4]) / 100.0; g_fprof[5] += (uint32_t)(fw[6] - fw[5]) / 100.0;
        g_fprof[6] += (uint32_t)(fw[7] - fw[6]) / 100.0; g_fprof[7] += 1;
        g_fprof[3] -= h3;             // (done-to-return: the return adds its time)
#endif
    } else if (rc == PP_ERR_STATE) {
        // a launch shape other than the one-launch step (debug shapes, maps beyond the LDS): copies
        if (hipMemcpyAsync(d, &h, sizeof(Frame), hipMemcpyHostToDevice, st) != hipSuccess) return PP_ERR_HIP;
        rc = eval_impl(M, &B, &P, &R, device, (void*)st, nullptr);
        if (rc == PP_OK && (hipMemcpyAsync(&h, d, sizeof(Frame), hipMemcpyDeviceToHost, st) != hipSuccess ||
                            hipStreamSynchronize(st) != hipSuccess))
            rc = PP_ERR_HIP;
    }
    if (rc != PP_OK) return rc;
    DS.plan_table.take_back(hs, 0, nslots);
    *n_out = h.nout;
    for (int i = 0; i < h.nout && i < N; i++) { next_x[i] = h.nx[i]; next_y[i] = h.ny[i]; }
    *target_lane = h.info.target_lane;
#ifdef PP_FRAME_PROF
    g_fprof[3] += fprof_now();
#endif
    return PP_OK;
}

}  // extern "C"
