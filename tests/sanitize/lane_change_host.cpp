// lane_change_host.cpp — lane-changing traffic's shared arithmetic (csrc/pp_lanechange.h, the function
// k_lane_change and pp_traffic_lane_change_host both call) as a stand-alone host program under
// AddressSanitizer and UndefinedBehaviorSanitizer (`make -C carnd-path-planning-project_amd
// sanitize-lane-change`, driven by tests/test_world_sanitize.py). Test infrastructure; never part
// of the product library.
//
// Every array is a std::vector of exactly the size include/pp.h states, so an index outside
// [k * S + s] is a heap overflow the sanitizer reports. On lane tables of a 16-waypoint ring:
//   overtake     a 20 m/s car 40 m behind a 10 m/s car on lane 1: the change to lane 0 by hand, the
//                position kept, the offset back home after the worked-out number of calls
//   random       seeded episodes: 0..20 cars anywhere on the ring (parked ones, identical positions),
//                the ego anywhere, any consume, random valid configurations, follow + lane change +
//                move per frame, states reused by zeroing `started`, scenes the follow update has not
//                started
// Exit 0 and a last line "clean" when every check passed; a sanitizer report aborts the process.
#include "world_fixture.h"
#include "../../carnd-path-planning-project_amd/csrc/pp_lanechange.h"

namespace {

constexpr int kWp = 16;

struct Change {                   // pp_lane_change over exactly sized vectors
    std::vector<int32_t> started, n_changes, last_car, last_dir, wait, changes, dir;
    std::vector<double> home, arc, gain;
    Change(int64_t S, int n)
        : started(S), n_changes(S), last_car(S), last_dir(S), wait(S * n), changes(S * n), dir(S * n), home(S * n),
          arc(S * n), gain(S * n) {}
    pp_lane_change view() {
        pp_lane_change l;
        l.started = started.data(); l.n_changes = n_changes.data(); l.last_car = last_car.data();
        l.last_dir = last_dir.data(); l.home = home.data(); l.wait = wait.data(); l.changes = changes.data();
        l.arc = arc.data(); l.gain = gain.data(); l.dir = dir.data();
        return l;
    }
};

pp_follow_cfg follow_cfg() { return default_of(ppfollow::cfg_default); }
pp_lane_change_cfg change_cfg() { return default_of(pplanechange::cfg_default); }

void frame(const Ring& R, const std::vector<double>& ex, const std::vector<double>& ey, const std::vector<double>& mph,
           Traffic& tr, int consume, const pp_follow_cfg& fc, FollowState& fo, const pp_lane_change_cfg& lc, Change& ch,
           bool with_follow = true) {
    const pp_follow f = fo.view();
    const pp_lane_change l = ch.view();
    const ppsynth::TrafficV tv = tr.view();
    for (int64_t s = 0; s < tr.S; s++) {
        if (with_follow) ppfollow::follow_scene(R.T, R.A, tr.S, s, ex[s], ey[s], mph[s], tv, consume, fc, f);
        pplanechange::lane_change_scene(R.T, R.A, tr.S, s, ex[s], ey[s], mph[s], tv, consume, fc, f, lc, l);
    }
}

void overtake(const Ring& R) {
    const int64_t S = 3;
    const pp_follow_cfg fc = follow_cfg();
    const pp_lane_change_cfg lc = change_cfg();
    const double L = R.T.seg_len[1 * kWp + 2];
    Traffic tr(S, 2);
    std::vector<double> ex(S), ey(S), mph(S, 10.0);
    for (int64_t s = 0; s < S; s++) {             // lane 1, segment 2: the fast car at 2 m, the slow one at 42 m
        tr.lane[0 * S + s] = 1; tr.seg[0 * S + s] = 2; tr.t[0 * S + s] = 2.0 / L; tr.v[0 * S + s] = 20.0;
        tr.lane[1 * S + s] = 1; tr.seg[1 * S + s] = 2; tr.t[1 * S + s] = 42.0 / L; tr.v[1 * S + s] = 10.0;
        tr.off[0 * S + s] = 0.25; tr.off[1 * S + s] = -0.1;
        R.point(NL - 1, 9, 0.5, 3.0, &ex[s], &ey[s]);   // the ego across the ring, outside the outermost lane
    }
    FollowState fo(S, 2);
    Change ch(S, 2);
    double x0, y0, x1, y1;
    R.point(1, 2, 2.0 / L, 0.25, &x0, &y0);
    frame(R, ex, ey, mph, tr, 3, fc, fo, lc, ch);
    // the follow update: net gap 35.5 m, s* = 2 + 24 + 20 * 10 / (2 sqrt 6); the change: a free road
    const double two_sab = 2 * sqrt(6.0), sstar = 2 + 24 + 200 / two_sab;
    const double a1 = 2.0 * (0 - (sstar / 35.5) * (sstar / 35.5));
    const double v1 = 20.0 + a1 * 0.06, r = v1 / 20.0;
    const double free = 1 - r * r * r * r, dyn = v1 * 1.2 + v1 * (v1 - 10.0) / two_sab;
    const double gain = 2.0 * free - 2.0 * (free - ((2 + dyn) / 35.5) * ((2 + dyn) / 35.5));
    int need = 0;
    for (int64_t s = 0; s < S; s++) {
        CHECK(fabs(tr.v[0 * S + s] - v1) < 1e-12 && tr.v[1 * S + s] == 10.0);
        CHECK(ch.last_car[s] == 1 && ch.last_dir[s] == -1 && ch.n_changes[s] == 1 && ch.started[s] == 1);
        CHECK(tr.lane[0 * S + s] == 0 && tr.lane[1 * S + s] == 1 && tr.seg[0 * S + s] == 2);
        CHECK(fabs(ch.gain[0 * S + s] - (gain - 0.2)) < 1e-9 && ch.dir[0 * S + s] == -1);
        CHECK(fabs(ch.gain[1 * S + s] - (0.3 * gain - 0.2)) < 1e-9);
        CHECK(ch.wait[0 * S + s] == 250 && ch.wait[1 * S + s] == 0 && ch.changes[0 * S + s] == 1 && ch.changes[1 * S + s] == 0);
        // (the chords of lanes 0 and 1 are parallel, 4 cos(pi / 16) m apart)
        CHECK(ch.home[0 * S + s] == 0.25 && fabs(tr.off[0 * S + s] - (0.25 + 4 * cos(kPi / kWp))) < 1e-9);
        R.point(0, tr.seg[0 * S + s], tr.t[0 * S + s], tr.off[0 * S + s], &x1, &y1);
        CHECK(fabs(x1 - x0) < 1e-9 && fabs(y1 - y0) < 1e-9);
        need = (int)ceil(fabs(tr.off[0 * S + s] - 0.25) / (1.5 * 0.06));
    }
    for (int k = 1; k <= need; k++) {
        frame(R, ex, ey, mph, tr, 3, fc, fo, lc, ch);
        for (int64_t s = 0; s < S; s++) {
            CHECK((tr.off[0 * S + s] == 0.25) == (k == need));
            CHECK(ch.last_car[s] == 0 && ch.gain[0 * S + s] == -INFINITY && ch.dir[0 * S + s] == 0);
            CHECK(tr.off[1 * S + s] == -0.1);
        }
    }
    printf("lane change: overtake by hand, home again after %d calls, %d scenes\n", need, (int)S);
}

void random_frames(const Ring& R, uint64_t seed, int rounds) {
    Rng g(seed);
    int frames = 0, begun = 0, skipped = 0;
    for (int r = 0; r < rounds; r++) {
        const int64_t S = 1 + g.below(7);
        const int n_cars = g.below(21);
        pp_follow_cfg fc = follow_cfg();
        if (g.below(2)) {
            fc.max_acc = g.uni(0.1, 5); fc.comfort_brake = g.uni(0.1, 6); fc.max_brake = g.uni(0.5, 12);
            fc.time_headway = g.uni(0, 3); fc.min_gap = g.uni(0, 5); fc.gap_floor = g.uni(0.01, 2);
            fc.horizon = g.below(4) ? g.uni(0, 400) : 1e9; fc.car_length = g.uni(0, 8); fc.ego_length = g.uni(0, 8);
            fc.lateral_reach = g.uni(0, 6); fc.react_to_ego = g.below(5) != 0;
        }
        pp_lane_change_cfg lc = change_cfg();
        lc.politeness = g.uni(0, 1); lc.threshold = g.below(8) ? g.uni(-0.5, 1) : INFINITY; lc.right_bias = g.uni(-0.5, 0.5);
        lc.safe_brake = g.uni(0.5, 9); lc.lateral_speed = g.uni(0.2, 4); lc.ego_desired_speed = g.uni(1, 30);
        lc.min_interval_steps = g.below(60);
        CHECK(ppfollow::cfg_ok(fc) && pplanechange::cfg_ok(lc));
        Traffic tr(S, n_cars);
        for (size_t k = 0; k < tr.lane.size(); k++) {
            tr.lane[k] = g.below(NL); tr.seg[k] = g.below(kWp); tr.t[k] = g.below(10) ? g.unit() : (double)g.below(2);
            tr.off[k] = g.uni(-1, 1); tr.v[k] = g.below(6) ? g.uni(0, 30) : 0.0;
            if (k >= (size_t)S && !g.below(10)) { tr.lane[k] = tr.lane[k - S]; tr.seg[k] = tr.seg[k - S]; tr.t[k] = tr.t[k - S]; }
        }
        FollowState fo(S, n_cars);
        Change ch(S, n_cars);
        const int n_frames = 1 + g.below(40);
        std::vector<double> ex(S), ey(S), mph(S);
        for (int64_t s = 0; s < S; s++) R.point(g.below(NL), g.below(kWp), g.unit(), g.uni(-3, 3), &ex[s], &ey[s]);
        if (!g.below(10)) {                        // the follow update has not run: the call leaves everything alone
            const Traffic before = tr;
            const Change was = ch;
            frame(R, ex, ey, mph, tr, 3, fc, fo, lc, ch, false);
            CHECK(before.lane == tr.lane && before.seg == tr.seg && before.t == tr.t && before.off == tr.off);
            CHECK(was.started == ch.started && was.gain == ch.gain && was.wait == ch.wait);
            skipped++;
        }
        for (int f = 0; f < n_frames; f++, frames++) {
            const int consume = 1 + g.below(9);
            for (int64_t s = 0; s < S; s++) {
                mph[s] = g.uni(0, 60);
                if (!g.below(6)) {                 // the ego jumps: anywhere, also far from every lane
                    const double a = g.uni(0, 2 * kPi), rad = g.below(4) ? g.uni(118, 136) : g.uni(0, 400);
                    ex[s] = rad * cos(a); ey[s] = rad * sin(a);
                    fo.started[s] = 0;             // (a jump beyond the hint's reach starts a new follow episode)
                }
            }
            const Traffic before = tr;
            const std::vector<int32_t> wait = ch.wait, total = ch.n_changes, was_started = ch.started;
            frame(R, ex, ey, mph, tr, consume, fc, fo, lc, ch);
            for (int64_t s = 0; s < S; s++) {
                CHECK(ch.started[s] == 1 || n_cars == 0);
                const int w = ch.last_car[s] - 1;
                CHECK(w >= -1 && w < n_cars && (w >= 0) == (ch.last_dir[s] != 0));
                CHECK(n_cars == 0 || ch.n_changes[s] == (was_started[s] ? total[s] : 0) + (w >= 0));
                begun += w >= 0;
                for (int j = 0; j < n_cars; j++) {
                    const size_t k = (size_t)j * S + s;
                    CHECK(tr.lane[k] >= 0 && tr.lane[k] < NL && tr.seg[k] >= 0 && tr.seg[k] < kWp);
                    CHECK(tr.t[k] >= 0 && tr.t[k] <= 1 + 1e-12 && ch.wait[k] >= 0);
                    CHECK(ch.dir[k] >= -1 && ch.dir[k] <= 1 && (ch.dir[k] == 0) == (ch.gain[k] == -INFINITY));
                    if (j == w) {
                        CHECK(tr.lane[k] == before.lane[k] + ch.last_dir[s] && ch.dir[k] == ch.last_dir[s] && ch.gain[k] > 0);
                        CHECK(ch.wait[k] == lc.min_interval_steps && fo.desired[k] > 0);
                        CHECK(!was_started[s] || wait[k] - consume <= 0);
                    } else {
                        CHECK(tr.lane[k] == before.lane[k] && tr.seg[k] == before.seg[k] && tr.t[k] == before.t[k]);
                        CHECK(fabs(tr.off[k] - ch.home[k]) <= fabs(before.off[k] - ch.home[k]));
                    }
                    CHECK(lc.threshold < INFINITY || ch.gain[k] == -INFINITY);
                }
            }
            move(R, tr, consume);
            if (f + 1 < n_frames && !g.below(15)) ch.started[g.below((int)S)] = 0;   // a scene starts a new episode
        }
    }
    CHECK(begun > 100 && skipped > 0);
    printf("lane change: %d random frames in %d episodes, %d changes begun, %d calls before any follow update\n", frames,
           rounds, begun, skipped);
}

}  // namespace

int main() {
    pp_lane_change_cfg bad = change_cfg();
    bad.politeness = -1;
    CHECK(!pplanechange::cfg_ok(bad));
    bad = change_cfg();
    bad.threshold = NAN;
    CHECK(!pplanechange::cfg_ok(bad));
    bad = change_cfg();
    bad.min_interval_steps = -1;
    CHECK(!pplanechange::cfg_ok(bad));
    CHECK(pplanechange::cfg_ok(change_cfg()));
    const Ring R(kWp, 120.0);
    overtake(R);
    random_frames(R, 20261020, 300);
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("clean\n");
    return 0;
}
