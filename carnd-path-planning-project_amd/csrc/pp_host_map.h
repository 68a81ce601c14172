// pp_host_map.h — host: the owners of device resources, pp_map, per-device state, per-stream
// workspace, the map tables and their upload. Part of pp_eval.hip's translation unit.
#pragma once

// ================================================================================================
// host side: map, per-device state, C-ABI
// ================================================================================================
namespace {

constexpr int kMaxDev = 16;
constexpr int kMaxWaypoints = 1 << 24;
constexpr int kPrepD = 12 + 4 * NL;   // doubles per scene in PrepV (see prep_bind)
constexpr int kPrepI = 7;

// The owners of device resources. Each is move-only and releases what it holds in reset() and in its
// destructor; nothing else in csrc/ frees device memory, pinned memory, a stream or an event.
template <class H, hipError_t (*kRelease)(H)>
class Owned {
    H h_ = nullptr;
public:
    Owned() = default;
    Owned(Owned&& o) noexcept { std::swap(h_, o.h_); }
    Owned& operator=(Owned&& o) noexcept { std::swap(h_, o.h_); return *this; }   // (o releases the old one)
    ~Owned() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) (void)kRelease(h_); h_ = nullptr; }
    H* out() { reset(); return &h_; }          // for the runtime's create calls
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
struct Pinned : Owned<void*, hipHostFree> {     // pinned host memory
    int alloc(size_t bytes, unsigned flags) {
        void* p = nullptr;
        const bool ok = hipHostMalloc(&p, bytes, flags) == hipSuccess;
        *out() = ok ? p : nullptr;
        if (!ok) (void)hipGetLastError();      // (as DevMem::grow)
        return ok ? PP_OK : PP_ERR_NOMEM;
    }
};
// device memory and the capacity it was grown to, in its user's unit (scenes, words, bytes): the two
// change only together
template <class T = void>
class DevMem {
    T* p_ = nullptr;
    int64_t cap_ = 0;
public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept { *this = std::move(o); }
    DevMem& operator=(DevMem&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }   // (o releases the old one)
    ~DevMem() { reset(); }
    T* get() const { return p_; }
    int64_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    // at least `cap` units (`bytes` for that many): a buffer too small is released once `st`, the
    // stream that uses it, has drained, and a new one made; its contents are not kept. A refused
    // allocation leaves the owner empty and takes the runtime's last error with it, so the next
    // call's launch check (hipGetLastError) does not report it.
    int grow(hipStream_t st, int64_t cap, size_t bytes) {
        if (cap_ >= cap) return PP_OK;
        if (p_) { (void)hipStreamSynchronize(st); reset(); }
        if (hipMalloc((void**)&p_, bytes) != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return PP_ERR_NOMEM; }
        cap_ = cap;
        return PP_OK;
    }
    int alloc(size_t n) { return grow(nullptr, (int64_t)n, sizeof(T) * n); }     // n elements, for an empty owner
};
// the timing events: the pool pp_eval takes from and the calls' records (raw handles: pp_timing_read
// indexes them)
struct EventSet {
    std::vector<hipEvent_t> pool;
    // groups of 4 kPartMax per pp_eval: before K1, after K1, after K2, after K3/K4 on the launch
    // stream (the split: those four per part, each part's on its own stream, events 4 h .. 4 h + 3)
    std::vector<hipEvent_t> rec;
    // per group: bit 0 K3/K4 launched, bit 4 K2's events only, bit 5 no K1 kernel (the one-launch
    // step), bits 8-15 the split's launched parts (0: none), bits 16-19 its parts per chunk (0: one chunk)
    std::vector<int> kind;
    EventSet() = default;
    EventSet(EventSet&& o) noexcept { *this = std::move(o); }
    EventSet& operator=(EventSet&& o) noexcept { pool.swap(o.pool); rec.swap(o.rec); kind.swap(o.kind); return *this; }
    ~EventSet() {
        for (auto* v : {&pool, &rec})
            for (hipEvent_t e : *v) { Event own; *own.out() = e; }
    }
};

// pp_eval's device workspaces, one set per HIP stream: evaluations on different streams never
// share intermediate buffers, and evaluations on one stream are ordered by it. A buffer is grown
// only after that stream has drained (it is the only stream using it).
// the split of shard-sized batches: parts (streams) per call, at most kSplitMax (split_parts)
constexpr int kSplitMax = 4;
// parts per call: a batch beyond kSplitMaxScenes runs as chunks of parts, part t on stream t % streams
// (split_chunks); each part has its own flagged-group count word and 4 timing-event slots
constexpr int kPartMax = 16;
// the persistent kernels' claim counters, behind the parts' count words (zeroed with them, on the
// stream, ahead of every call's K1): word 0 the persistent k_cand's
constexpr int kPersistCtr = 2;
struct StreamWS {
    DevMem<> ws;                  // prep workspace (capacity: evaluations, scene x draw)
    DevMem<> rec;                 // reference-mode winner record (capacity: scenes)
    DevMem<uint32_t> gbits;       // k_cand groups holding a kLimSlow scene (bitmap; all zero between calls; capacity: words)
    DevMem<> srt;                 // k_sort_cars' visit-major rows (SortedCars; capacity: bytes)
    DevMem<> sum;                 // the judge summary's chunk parts and tile sums (SumRecs; capacity: bytes)
    Stream st2[kSplitMax - 1];    // the split's other streams (shard-sized batches)
    Event fork, join[kSplitMax - 1];
};
// the device copies of the map's tables (dev_init, pp_map_create_device)
struct DevTables {
    DevMem<double> map;           // kMapArrays * n
    DevMem<double> lanetab;       // synth tables: lc_x[NL n] lc_y[NL n] seg_len[NL n] tan_x[NL n] tan_y[NL n]
    DevMem<uint2> wgrid;          // the closest-waypoint cell table (pp_map::wgrid)
    DevMem<double2> wseg;         // reference segment lengths and reciprocals (pp_map::wseg)
    DevMem<double> atab;          // the approach table (pp_map::atab)
};
// everything a map holds on one device. pp_map_destroy releases it by assigning an empty one while
// the device is current and idle; init is true from the first successful dev_init on.
struct DevRes {
    bool init = false;
    DevTables tab;
    DevMem<double> arctab;        // pp_map::arctab, uploaded on the first follow call (arc_init)
    std::map<void*, StreamWS> sws;  // per hip_stream
    DevMem<> frame;               // single-frame scratch (pp_plan_frame)
    Pinned frame_host;            // its pinned host staging copy (coherent: k_plan_frame reads and
                                  // writes it; the frame's done word follows the frame)
    Stream frame_stream;          // pp_plan_frame's stream
    DevMem<> stage;               // pp_plan_batch_host staging buffer (capacity: bytes)
    Pinned stage_host;            // its pinned host mirror (one copy per direction and region)
    EventSet ev;
};
struct DevState : DevRes {
    uint32_t frame_seq = 0;       // the last frame's done word
    std::mutex frame_mu;          // one pp_plan_frame at a time per device (frame scratch + car table)
    std::mutex stage_mu;          // one pp_plan_batch_host at a time per device
    pptab::CarTable plan_table;   // pp_plan_frame's persistent car table (the reference's std::map)
    int timing = 0;               // pp_timing_enable: 0 off, 1 every kernel, 2 K2 only
    // the persistent k_cand's resident blocks on this device (occupancy query x CUs), asked once
    // per launch geometry (threads, LDS bytes); 0: not asked yet
    int persist_blocks = 0, persist_threads = 0;
    size_t persist_lds = 0;
};

}  // namespace

struct pp_map {
    int n = 0;
    std::vector<double> geom;     // kMapArrays * n (MapG layout)
    std::vector<double> ptab;     // (4 + 2 NL) * n: ref xy, normal, lane centres (pp_map_geometry)
    std::vector<double> lanetab;  // 5 NL * n
    std::vector<double> arctab;   // reactive traffic's arc prefix (ppfollow::build_arc): cum[NL n] loop[NL]
    int fastm = 0;                // MapV::fastm: bit 1: every lane segment's rdenom in [2^-500, 2^500]; bit 2: approach_seg's map bounds
    std::vector<uint2> wgrid;     // closest-waypoint cell table (build_wgrid; empty: none)
    std::vector<double2> wseg;    // reference segment lengths and reciprocals (build_wseg; empty: none)
    std::vector<double> atab;     // lane matching's approach table (build_atab; empty: none)
    WGrid wg;                     // its geometry (cells: the device copy, set per device)
    DevState dev[kMaxDev];
    std::mutex mu;
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(d); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// reactive traffic's arc prefix from the host lanetab's seg_len (for a pp_map_create_device map: the
// mirrored device values), one left-to-right sum per lane
void fill_arctab(pp_map* M) {
    M->arctab.assign(ppfollow::arc_doubles(M->n), 0.0);
    ppfollow::build_arc(M->lanetab.data() + 2 * NL * (size_t)M->n, M->n, M->arctab.data());
}

// pp_map_geometry's table from the MapG layout: per waypoint ref xy, normal, lane centres
void fill_ptab(pp_map* M) {
    const int n = M->n;
    const double* g = M->geom.data();
    M->ptab.assign((4 + 2 * NL) * (size_t)n, 0.0);
    for (int i = 0; i < n; i++) {
        double* o = &M->ptab[(4 + 2 * NL) * (size_t)i];
        o[0] = g[i]; o[1] = g[n + i]; o[2] = g[2 * n + i]; o[3] = g[3 * n + i];
        for (int r = 0; r < NL; r++) { o[4 + 2 * r] = g[(4 + r) * n + i]; o[5 + 2 * r] = g[(4 + NL + r) * n + i]; }
    }
    M->fastm = 1;
    for (size_t i = (size_t)(4 + 3 * NL) * n; i < (size_t)(4 + 4 * NL) * n; i++)
        if (!(g[i] >= 0x1p-500 && g[i] <= 0x1p500)) M->fastm = 0;
    // bit 2 (lane matching's approach runs, pp_device.h approach_seg): every lane segment's rdenom
    // >= 1 m^2 and every lane centre within 4e4 m of the origin
    bool appr = M->fastm != 0;
    for (size_t i = (size_t)(4 + 3 * NL) * n; i < (size_t)(4 + 4 * NL) * n; i++) appr = appr && g[i] >= 1.0;
    for (size_t i = (size_t)4 * n; i < (size_t)(4 + 2 * NL) * n; i++) appr = appr && std::fabs(g[i]) < 4e4;
    if (appr) M->fastm |= 2;
}

// The closest-waypoint cell table (pp_device.h WGrid, init_reference_waypoint). Cells of 16 m
// within 32 m of the waypoint polyline get a list: waypoint w can be the closest one to a point of
// cell B only if its distance to B, dmin(w, B), is at most U = min over all waypoints of the
// largest distance from w' to B (the closest waypoint of any point of B is at most U away). B is
// grown by 0.5 m on each side (the kernel's cell index rounds), and the test carries a relative
// margin of 1e-6 (the kernel's squared distances round by a few ulps): the list holds every
// waypoint that can be the scan's answer. Lists of up to 4 (the highway map's cells near the road
// hold 1-4); a cell with more, or away from the road, has none (0xFFFFFFFF: the kernel scans).
// Maps of more than 65,535 waypoints, or whose table would take more than 5e7 distance tests to
// build, get no table.
constexpr double kWgridMaxCells = 4e6;
void build_wgrid(pp_map* M) {
    constexpr double kCell = 16.0, kNear = 32.0, kGrow = 0.5;
    const int n = M->n;
    M->wgrid.clear();
    M->wg = WGrid{};
    if (n < 1 || n > 65535) return;
    const double* rx = M->geom.data();
    const double* ry = rx + n;
    double x0 = rx[0], x1 = rx[0], y0 = ry[0], y1 = ry[0];
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(rx[i]) || !std::isfinite(ry[i])) return;
        x0 = std::min(x0, rx[i]); x1 = std::max(x1, rx[i]); y0 = std::min(y0, ry[i]); y1 = std::max(y1, ry[i]);
    }
    const double gx0 = x0 - 2 * kNear, gy0 = y0 - 2 * kNear;
    const double wdt = x1 - x0 + 4 * kNear, hgt = y1 - y0 + 4 * kNear;
    if (!(wdt / kCell < 1e5 && hgt / kCell < 1e5)) return;
    const int gnx = (int)std::ceil(wdt / kCell), gny = (int)std::ceil(hgt / kCell);
    // at most 4e6 cells (a 32 km square; 32 MB on the host and the device): a map spread wider
    // keeps the full scan (two waypoints 1,000 km apart would ask for ~4e9 cells)
    if ((double)gnx * (double)gny > kWgridMaxCells) return;
    // cells near the polyline: sample every segment every 2 m, mark cells within kNear
    std::vector<uint8_t> near((size_t)gnx * gny, 0);
    const int R = (int)std::ceil(kNear / kCell);
    for (int i = 0; i < n; i++) {
        const int j = (i + 1) % n;
        const double len = std::hypot(rx[j] - rx[i], ry[j] - ry[i]);
        const int ns = std::max(1, (int)std::ceil(len / 2.0));
        for (int k = 0; k <= ns; k++) {
            const double t = (double)k / ns;
            const double px = rx[i] + (rx[j] - rx[i]) * t, py = ry[i] + (ry[j] - ry[i]) * t;
            const int ci = (int)((px - gx0) / kCell), cj = (int)((py - gy0) / kCell);
            for (int dj = -R; dj <= R; dj++)
                for (int di = -R; di <= R; di++) {
                    const int a = ci + di, b = cj + dj;
                    if (a >= 0 && b >= 0 && a < gnx && b < gny) near[(size_t)b * gnx + a] = 1;
                }
        }
    }
    size_t nnear = 0;
    for (uint8_t v : near) nnear += v;
    if ((double)nnear * n > 5e7) return;
    std::vector<uint2> cells((size_t)gnx * gny, uint2{0xFFFFFFFFu, 0xFFFFFFFFu});
    std::vector<int> cand;
    for (int cj = 0; cj < gny; cj++)
        for (int ci = 0; ci < gnx; ci++) {
            if (!near[(size_t)cj * gnx + ci]) continue;
            const double bx0 = gx0 + ci * kCell - kGrow, bx1 = gx0 + (ci + 1) * kCell + kGrow;
            const double by0 = gy0 + cj * kCell - kGrow, by1 = gy0 + (cj + 1) * kCell + kGrow;
            double U = INFINITY;
            for (int i = 0; i < n; i++) {
                const double fx = std::max(std::fabs(rx[i] - bx0), std::fabs(rx[i] - bx1));
                const double fy = std::max(std::fabs(ry[i] - by0), std::fabs(ry[i] - by1));
                U = std::min(U, fx * fx + fy * fy);
            }
            const double lim = U * (1 + 1e-6) + 1e-6;
            cand.clear();
            for (int i = 0; i < n && cand.size() <= 4; i++) {
                const double dx = std::max({bx0 - rx[i], rx[i] - bx1, 0.0});
                const double dy = std::max({by0 - ry[i], ry[i] - by1, 0.0});
                if (dx * dx + dy * dy <= lim) cand.push_back(i);
            }
            if (cand.empty() || cand.size() > 4) continue;
            while (cand.size() < 4) cand.push_back(cand.back());
            cells[(size_t)cj * gnx + ci] = uint2{(uint32_t)cand[0] | ((uint32_t)cand[1] << 16),
                                                 (uint32_t)cand[2] | ((uint32_t)cand[3] << 16)};
        }
    M->wgrid.swap(cells);
    M->wg.gx0 = gx0; M->wg.gy0 = gy0; M->wg.ginv = 1.0 / kCell; M->wg.gnx = gnx; M->wg.gny = gny;
}

// Map::project_speed's segment length (src/main.cpp:332-339: w = ref_b - ref_{b-1}, |w| =
// sqrt(wx^2 + wy^2), the same operations as the kernel, unfused, correctly rounded sqrt) and
// RN(1 / |w|) by IEEE division, per segment b (project_speed then divides by the reciprocal with one
// Markstein correction: the correctly rounded quotient, ppd::div_by_rcp). Only for maps whose
// lengths all lie in [2^-500, 2^500] (div_by_rcp's divisor range); else none.
void build_wseg(pp_map* M) {
    const int n = M->n;
    M->wseg.clear();
    const double* rx = M->geom.data();
    const double* ry = rx + n;
    std::vector<double2> t(n);
    for (int b = 0; b < n; b++) {
        const int a = (int)(((int64_t)b - 1 + n) % n);
        const double wx = rx[b] - rx[a], wy = ry[b] - ry[a];
        const double wvl = std::sqrt(wx * wx + wy * wy);
        if (!(wvl >= 0x1p-500 && wvl <= 0x1p500)) return;
        t[b] = double2{wvl, 1.0 / wvl};
    }
    M->wseg.swap(t);
}

// Lane matching's approach table (pp_device.h approach_cert): per lane segment b (waypoint b - 1 to
// b) and lane l, d = RN(pb - pa) (the walk's own differences), c = pa.d, and the certain test's
// constants c + rdenom + kAtabMargin (forward) and c - 1 - kAtabMargin (backward), rdenom the map's
// own table value. Only for maps with fastm bit 2 (the bounds its margin argument needs).
void build_atab(pp_map* M) {
    M->atab.clear();
    if (!(M->fastm & 2)) return;
    const int n = M->n;
    const double* g = M->geom.data();
    const double* lcx = g + 4 * (size_t)n;
    const double* lcy = g + (4 + NL) * (size_t)n;
    const double* llen = g + (4 + 2 * NL) * (size_t)n;
    const double* lden = g + (4 + 3 * NL) * (size_t)n;
    std::vector<double> t((size_t)kAtabD * n, 0.0);
    for (int b = 0; b < n; b++) {
        const int a = b == 0 ? n - 1 : b - 1;
        double* r = &t[(size_t)kAtabD * b];
        for (int l = 0; l < NL; l++) {
            const double pax = lcx[(size_t)l * n + a], pay = lcy[(size_t)l * n + a];
            const double dx = lcx[(size_t)l * n + b] - pax, dy = lcy[(size_t)l * n + b] - pay;
            const double c = pax * dx + pay * dy;
            r[2 * l] = dx;
            r[2 * l + 1] = dy;
            r[2 * NL + l] = c + lden[(size_t)l * n + b] + kAtabMargin;
            r[3 * NL + l] = c - 1.0 - kAtabMargin;
            r[4 * NL + l] = llen[(size_t)l * n + b];
        }
    }
    M->atab.swap(t);
}

// The optional per-map tables (cell table, segment reciprocals, approach table) speed K1 up and
// never change a result: a map whose tables cannot be built (an allocation failure included) runs
// without them. Nothing here throws across the C-ABI.
void build_tables(pp_map* M) {
    try { build_wgrid(M); } catch (...) { M->wgrid.clear(); M->wgrid.shrink_to_fit(); M->wg = WGrid{}; }
    try { build_wseg(M); } catch (...) { M->wseg.clear(); M->wseg.shrink_to_fit(); }
    try { build_atab(M); } catch (...) { M->atab.clear(); M->atab.shrink_to_fit(); }
}

// the device copy of a host array (an empty array: none). PP_ERR_NOMEM for the allocation,
// PP_ERR_HIP for the copy; `d` holds the copy only on PP_OK
template <class T>
int upload(DevMem<T>& d, const std::vector<T>& h) {
    d.reset();
    if (h.empty()) return PP_OK;
    const int rc = d.alloc(h.size());
    if (rc) return rc;
    if (hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) == hipSuccess) return PP_OK;
    d.reset();
    return PP_ERR_HIP;
}

// the device copies of the cell table, the segment table and the approach table (dev_init,
// pp_map_create_device)
int upload_wgrid(const pp_map* M, DevTables& T) {
    int rc = upload(T.wgrid, M->wgrid);
    if (!rc) rc = upload(T.wseg, M->wseg);
    if (!rc) rc = upload(T.atab, M->atab);
    return rc;
}

// Map::Init (src/main.cpp:89-131) + derived tables, on the host (done once per map).
int build_map(pp_map* M, const double* wx, const double* wy, int n) {
    M->n = n;
    std::vector<double> nx(n), ny(n), lcx(NL * n), lcy(NL * n);
    auto W = [n](int i) { return (int)(((int64_t)i + n) % n); };
    for (int i = 0; i < n; i++) {
        const int p = W(i - 1);
        const double dx = wx[i] - wx[p], dy = wy[i] - wy[p];
        const double len = std::sqrt(dx * dx + dy * dy);
        if (!(len > 0)) return PP_ERR_ARG;    // duplicate consecutive waypoints: Map::Init divides by 0
        nx[i] = dy / len;
        ny[i] = -dx / len;
    }
    for (int i = 0; i < n; i++) {
        const int q = W(i + 1);
        double ax = (nx[i] + nx[q]) / 2, ay = (ny[i] + ny[q]) / 2;
        const double a_n = std::atan2(ny[i], nx[i]);
        const double a_avg = std::atan2(ay, ax);
        const double cos_alpha = std::cos(a_avg - a_n);
        ax /= cos_alpha;
        ay /= cos_alpha;
        for (int r = 0; r < NL; r++) {
            const double off = 4.0 * (r + 0.5);
            lcx[r * n + i] = wx[i] + ax * off;
            lcy[r * n + i] = wy[i] + ay * off;
        }
    }
    M->geom.assign(kMapArrays * (size_t)n, 0.0);
    double* g = M->geom.data();
    for (int i = 0; i < n; i++) {
        g[i] = wx[i]; g[n + i] = wy[i]; g[2 * n + i] = nx[i]; g[3 * n + i] = ny[i];
        for (int r = 0; r < NL; r++) {
            g[(4 + r) * n + i] = lcx[r * n + i];
            g[(4 + NL + r) * n + i] = lcy[r * n + i];
            const int p = W(i - 1);
            const double dx = lcx[r * n + i] - lcx[r * n + p], dy = lcy[r * n + i] - lcy[r * n + p];
            g[(4 + 2 * NL + r) * n + i] = std::sqrt(dx * dx + dy * dy);    // Map::get_lane_length
            const double ex = lcx[r * n + p] - lcx[r * n + i], ey = lcy[r * n + p] - lcy[r * n + i];
            const double den = ex * ex + ey * ey;                           // helpers.h:202 rdenom
            g[(4 + 3 * NL + r) * n + i] = den;
            g[(4 + 4 * NL + r) * n + i] = 1.0 / den;
        }
    }
    fill_ptab(M);
    build_tables(M);
    M->lanetab.assign(5 * NL * (size_t)n, 0.0);
    double* t = M->lanetab.data();
    for (int r = 0; r < NL; r++)
        for (int i = 0; i < n; i++) {
            const double len = g[(4 + 2 * NL + r) * n + i];
            const int p = W(i - 1);
            t[0 * NL * n + r * n + i] = lcx[r * n + i];
            t[1 * NL * n + r * n + i] = lcy[r * n + i];
            t[2 * NL * n + r * n + i] = len;
            t[3 * NL * n + r * n + i] = (lcx[r * n + i] - lcx[r * n + p]) / len;
            t[4 * NL * n + r * n + i] = (lcy[r * n + i] - lcy[r * n + p]) / len;
        }
    fill_arctab(M);
    return PP_OK;
}

ppsynth::OutBatch out_batch(const pp_scene_batch* b) {
    ppsynth::OutBatch o;
    o.S = b->n_scenes;
    o.ego_x = (double*)b->ego_x; o.ego_y = (double*)b->ego_y;
    o.ego_yaw_deg = (double*)b->ego_yaw_deg; o.ego_speed_mph = (double*)b->ego_speed_mph;
    o.prev_x = (double*)b->prev_x; o.prev_y = (double*)b->prev_y;
    o.n_prev = (int32_t*)b->n_prev; o.prev_target_lane = (int32_t*)b->prev_target_lane;
    o.n_cars = (int32_t*)b->n_cars; o.car_id = (int32_t*)b->car_id;
    o.car_x = (double*)b->car_x; o.car_y = (double*)b->car_y;
    o.car_vx = (double*)b->car_vx; o.car_vy = (double*)b->car_vy;
    return o;
}

bool traffic_ok(const pp_traffic* t, const pp_scene_batch* b) {
    return t && b && t->n_cars >= 0 && t->n_cars <= PP_MAX_CARS && t->lane && t->seg && t->t &&
           t->offset && t->speed;
}

// a stage's state has every array (the pointers only); *_ok: that and a configuration in range
bool judge_state_ok(const pp_judge* j) {
    return j && j->steps && j->flags && j->count && j->first_step && j->first_car && j->seg_hint && j->off_run &&
           j->head_x && j->head_y && j->ring_vx && j->ring_vy && j->dist && j->clean_dist && j->min_sep &&
           j->max_speed_mph && j->max_acc && j->max_jerk;
}
bool judge_ok(const pp_judge_cfg* c, const pp_judge* j) { return c && ppjudge::cfg_ok(*c) && judge_state_ok(j); }

// what the judge reads of a frame: the ego pose, the traffic, the plan
bool judge_frame_ok(const pp_scene_batch* tel, const pp_traffic* traffic, const pp_result* plan, int32_t consume) {
    return tel && plan && tel->n_scenes >= 0 && tel->ego_x && tel->ego_y && tel->ego_yaw_deg &&
           traffic_ok(traffic, tel) && plan->n_out && plan->next_x && plan->next_y && consume >= 1;
}

bool follow_state_ok(const pp_follow* f) {
    return f && f->started && f->ego_seg && f->desired && f->next_speed && f->leader && f->gap;
}
bool follow_ok(const pp_follow_cfg* c, const pp_follow* f) { return c && ppfollow::cfg_ok(*c) && follow_state_ok(f); }

// what the follow update reads of a frame: the ego's position and speed, the traffic
bool follow_frame_ok(const pp_scene_batch* tel, const pp_traffic* traffic, int32_t consume) {
    return tel && tel->n_scenes >= 0 && tel->ego_x && tel->ego_y && tel->ego_speed_mph &&
           traffic_ok(traffic, tel) && consume >= 1;
}

bool lane_change_ok(const pp_lane_change_cfg* c, const pp_lane_change* l) {
    return c && l && pplanechange::cfg_ok(*c) && l->started && l->n_changes && l->last_car && l->last_dir &&
           l->home && l->wait && l->changes && l->arc && l->gain && l->dir;
}

// the sensor's configuration in range and every array of its state (the row arrays where rows > 0)
bool sensor_ok(const pp_sensor_cfg* c, const pp_sensor* x, int32_t rows) {
    if (!c || !x || !ppsensor::cfg_ok(*c) || !x->frame || !x->n_cars) return false;
    return rows == 0 || (x->car_id && x->car_x && x->car_y && x->car_vx && x->car_vy && x->fate);
}

// what the sensor reads of a frame: the ego's position and the car rows
bool sense_frame_ok(const pp_scene_batch* tel) {
    if (!tel || tel->n_scenes < 0 || tel->car_stride < 0 || tel->car_stride > PP_MAX_CARS || !tel->ego_x ||
        !tel->ego_y || !tel->n_cars)
        return false;
    return tel->car_stride == 0 || (tel->car_id && tel->car_x && tel->car_y && tel->car_vx && tel->car_vy);
}

// the tracker's configuration in range and every array of its state (the slot and row arrays where rows > 0)
bool tracker_ok(const pp_tracker_cfg* c, const pp_tracker* x, int32_t rows) {
    if (!c || !x || !pptracker::cfg_ok(*c) || !x->frame || !x->n_tracks || !x->n_cars) return false;
    return rows == 0 || (x->id && x->misses && x->x && x->y && x->vx && x->vy && x->ppp && x->ppv && x->pvv &&
                         x->car_id && x->car_x && x->car_y && x->car_vx && x->car_vy && x->src);
}

ppsensor::Truth truth_view(const pp_scene_batch* b) {
    return {b->n_scenes, b->car_stride, b->ego_x, b->ego_y, b->n_cars, b->car_id, b->car_x, b->car_y, b->car_vx,
            b->car_vy};
}

ppsynth::TrafficV traffic_view(const pp_traffic* t, int64_t S) {
    ppsynth::TrafficV v;
    v.S = S; v.n = t->n_cars; v.lane = t->lane; v.seg = t->seg; v.t = t->t; v.off = t->offset; v.v = t->speed;
    return v;
}

ppsynth::LaneTables lane_tables(const double* t, int n) {
    ppsynth::LaneTables T;
    T.n = n; T.lc_x = t; T.lc_y = t + NL * n; T.seg_len = t + 2 * NL * n; T.tan_x = t + 3 * NL * n;
    T.tan_y = t + 4 * NL * n;
    return T;
}

int dev_init(pp_map* M, int device) {
    DevState& D = M->dev[device];
    if (D.init) return PP_OK;
    DevTables T;                  // all or nothing: a failing return releases what was made
    int rc = upload(T.map, M->geom);
    if (!rc) rc = upload(T.lanetab, M->lanetab);
    if (!rc) rc = upload_wgrid(M, T);
    if (rc) return rc;
    D.tab = std::move(T);
    D.init = true;
    return PP_OK;
}

// the device copy of the arc prefix, made on the first follow call on this device (after dev_init,
// under M->mu)
int arc_init(pp_map* M, int device) {
    DevState& D = M->dev[device];
    return D.arctab ? PP_OK : upload(D.arctab, M->arctab);
}

// The world stages' two table views. host_tables: over the map's host arrays, for the host twins.
struct WorldTables {
    ppsynth::LaneTables T;
    ppfollow::ArcTables AT;
};
WorldTables host_tables(const pp_map* M) {
    return {lane_tables(M->lanetab.data(), M->n), ppfollow::arc_tables(M->arctab.data(), M->n)};
}
// The same over the device copies, for a world kernel's launch: makes `device` current for its own
// lifetime and, under M->mu, uploads what is missing (the arc prefix only where want_arc; AT is null
// without it). rc: PP_OK, or why there are no tables.
struct WorldDev : WorldTables {
    DeviceGuard g;
    int rc;
    WorldDev(pp_map* M, int device, bool want_arc) : WorldTables{{}, {nullptr, nullptr}}, g(device) {
        std::lock_guard<std::mutex> lk(M->mu);
        rc = dev_init(M, device);
        if (!rc && want_arc) rc = arc_init(M, device);
        if (rc) return;
        T = lane_tables(M->dev[device].tab.lanetab.get(), M->n);
        if (want_arc) AT = ppfollow::arc_tables(M->dev[device].arctab.get(), M->n);
    }
};

// a kernel of one lane per scene in blocks of 256 on `st`; PP_ERR_HIP where the launch is refused
template <class K, class... Args>
int launch_scenes(K kernel, int64_t S, void* st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, (hipStream_t)st, args...);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

}  // namespace
