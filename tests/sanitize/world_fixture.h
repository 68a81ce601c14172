// world_fixture.h — what the stand-alone sanitizer programs of the rollout's world stages share
// (judge_host.cpp, follow_host.cpp, lane_change_host.cpp, episode_host.cpp): the check macro, a seeded
// generator, lane tables of a ring road, and the traffic, follow state and judge state of include/pp.h
// over std::vectors of exactly the stated sizes, so an index outside [k * S + s] is a heap overflow
// the sanitizer reports. Includes the stages' shared arithmetic as host code. Test infrastructure;
// never part of the product library.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define PP_HD
#include "../../include/pp.h"
#include "../../carnd-path-planning-project_amd/csrc/pp_synth.h"
#include "../../carnd-path-planning-project_amd/csrc/pp_follow.h"

inline int g_fail = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
    } while (0)

struct Rng {                      // xorshift64*: seeded, reproducible
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    int below(int n) { return n > 0 ? (int)(next() % (uint64_t)n) : 0; }
    double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double uni(double lo, double hi) { return lo + (hi - lo) * unit(); }
};

constexpr int NL = PP_NUM_LANES;
constexpr double kPi = 3.14159265358979323846;

// a product default configuration by value: default_of(ppfollow::cfg_default)
template <class Cfg>
Cfg default_of(void (*fill)(Cfg*)) {
    Cfg c;
    fill(&c);
    return c;
}

// lane tables of a ring of n waypoints, `radius` metres, driven counter-clockwise: lane r's centre
// 4 (r + 0.5) m to the right of the waypoints (outside); and their arc prefix
struct Ring {
    int n;
    std::vector<double> t, arc;
    ppsynth::LaneTables T;
    ppfollow::ArcTables A;
    double min_loop;              // the shortest lane's way round
    Ring(int n_, double radius) : n(n_), t((size_t)5 * NL * n_), arc(ppfollow::arc_doubles(n_)) {
        double* lx = t.data();
        double* ly = lx + NL * n;
        double* sl = ly + NL * n;
        double* tx = sl + NL * n;
        double* ty = tx + NL * n;
        for (int l = 0; l < NL; l++)
            for (int i = 0; i < n; i++) {
                const double r = radius + 4.0 * (l + 0.5), a = 2 * kPi * i / n;
                lx[l * n + i] = r * cos(a);
                ly[l * n + i] = r * sin(a);
            }
        for (int l = 0; l < NL; l++)
            for (int i = 0; i < n; i++) {
                const int p = i == 0 ? n - 1 : i - 1;
                const double dx = lx[l * n + i] - lx[l * n + p], dy = ly[l * n + i] - ly[l * n + p];
                const double len = sqrt(dx * dx + dy * dy);
                sl[l * n + i] = len;
                tx[l * n + i] = dx / len;
                ty[l * n + i] = dy / len;
            }
        T.n = n; T.lc_x = lx; T.lc_y = ly; T.seg_len = sl; T.tan_x = tx; T.tan_y = ty;
        ppfollow::build_arc(sl, n, arc.data());
        A = ppfollow::arc_tables(arc.data(), n);
        min_loop = A.loop[0];
        for (int l = 1; l < NL; l++) min_loop = A.loop[l] < min_loop ? A.loop[l] : min_loop;
    }
    // the point t of the way along segment seg of lane l, lat metres to the right
    void point(int l, int seg, double t, double lat, double* x, double* y) const {
        const int p = seg == 0 ? n - 1 : seg - 1;
        const double ax = T.lc_x[l * n + p], ay = T.lc_y[l * n + p];
        const double ux = T.tan_x[l * n + seg], uy = T.tan_y[l * n + seg];
        *x = ax + (T.lc_x[l * n + seg] - ax) * t + uy * lat;
        *y = ay + (T.lc_y[l * n + seg] - ay) * t - ux * lat;
    }
};

struct Traffic {                  // pp_traffic
    int64_t S;
    int n;
    std::vector<int32_t> lane, seg;
    std::vector<double> t, off, v;
    Traffic(int64_t S_, int n_) : S(S_), n(n_), lane(S_ * n_), seg(S_ * n_), t(S_ * n_), off(S_ * n_), v(S_ * n_) {}
    ppsynth::TrafficV view() {
        ppsynth::TrafficV tv;
        tv.S = S; tv.n = n; tv.lane = lane.data(); tv.seg = seg.data(); tv.t = t.data(); tv.off = off.data(); tv.v = v.data();
        return tv;
    }
};

// the traffic after a frame of `consume` steps at its speeds
inline void move(const Ring& R, Traffic& tr, int consume) {
    for (size_t k = 0; k < tr.lane.size(); k++)
        ppsynth::lane_advance(R.T, tr.lane[k], &tr.seg[k], &tr.t[k], tr.v[k] * 0.02 * consume);
}

struct FollowState {              // pp_follow; started0, seg0: what the per-scene words start as
    std::vector<int32_t> started, ego_seg, leader;
    std::vector<double> desired, next_speed, gap;
    FollowState(int64_t S, int n, int32_t started0 = 0, int32_t seg0 = 0)
        : started(S, started0), ego_seg(S, seg0), leader(S * n), desired(S * n), next_speed(S * n), gap(S * n) {}
    pp_follow view() {
        pp_follow f;
        f.started = started.data(); f.ego_seg = ego_seg.data(); f.desired = desired.data();
        f.next_speed = next_speed.data(); f.leader = leader.data(); f.gap = gap.data();
        return f;
    }
};

struct JudgeState {               // pp_judge; fill: what every element starts as
    std::vector<int32_t> steps, count, first_step, first_car, seg_hint, off_run;
    std::vector<uint32_t> flags;
    std::vector<double> head_x, head_y, ring_vx, ring_vy, dist, clean_dist, min_sep, max_speed_mph, max_acc, max_jerk;
    explicit JudgeState(int64_t S, int fill = 0)
        : steps(S, fill), count(PP_INC_KINDS * S, fill), first_step(PP_INC_KINDS * S, fill), first_car(S, fill),
          seg_hint(S, fill), off_run(S, fill), flags(S, (uint32_t)fill), head_x(S, fill), head_y(S, fill),
          ring_vx(PP_JUDGE_RING * S, fill), ring_vy(PP_JUDGE_RING * S, fill), dist(S, fill), clean_dist(S, fill),
          min_sep(S, fill), max_speed_mph(S, fill), max_acc(S, fill), max_jerk(S, fill) {}
    pp_judge view() {
        pp_judge j;
        j.steps = steps.data(); j.flags = flags.data(); j.count = count.data(); j.first_step = first_step.data();
        j.first_car = first_car.data(); j.seg_hint = seg_hint.data(); j.off_run = off_run.data();
        j.head_x = head_x.data(); j.head_y = head_y.data(); j.ring_vx = ring_vx.data(); j.ring_vy = ring_vy.data();
        j.dist = dist.data(); j.clean_dist = clean_dist.data(); j.min_sep = min_sep.data();
        j.max_speed_mph = max_speed_mph.data(); j.max_acc = max_acc.data(); j.max_jerk = max_jerk.data();
        return j;
    }
    template <class V> static bool eq(const V& a, const V& b) {
        return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
    }
    bool same(const JudgeState& o) const {        // every field, bit for bit
        return eq(steps, o.steps) && eq(count, o.count) && eq(first_step, o.first_step) && eq(first_car, o.first_car) &&
               eq(seg_hint, o.seg_hint) && eq(off_run, o.off_run) && eq(flags, o.flags) && eq(head_x, o.head_x) &&
               eq(head_y, o.head_y) && eq(ring_vx, o.ring_vx) && eq(ring_vy, o.ring_vy) && eq(dist, o.dist) &&
               eq(clean_dist, o.clean_dist) && eq(min_sep, o.min_sep) && eq(max_speed_mph, o.max_speed_mph) &&
               eq(max_acc, o.max_acc) && eq(max_jerk, o.max_jerk);
    }
};
