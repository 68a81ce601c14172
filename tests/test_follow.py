"""Reactive traffic (include/pp.h pp_traffic_follow, pp_rollout_reactive; csrc/pp_follow.h): every
traffic car follows the vehicle ahead of it in its lane, the ego included, by the Intelligent
Driver Model.

The definitions are the project's own (DESIGN.md "Reactive traffic"); the reference has no
simulator, so nothing here is compared with it. The oracle is the NumPy restatement below, written
independently of the library's code: arcs from a cumulative sum of the polyline lengths of
pp_map_geometry, the ego projected on every segment of every lane (no hint), the leader as the
argmin over a full [car, candidate] gap matrix (no loop, no staging), the speeds in one vectorised
expression.

Tolerances. `leader` is exact. `gap`, `speed` and `desired` within TOL = 1e-8 (test_judge's): one
frame is a few dozen roundings of magnitudes <= 1e4 m (arcs up to 7e3 m carry 1e-12 m; the gap
ratio squared times max_acc times dt stays below 1e-9 even at the gap floor). In the random frames
a car whose ORACLE decision lies within world_lib.FOLLOW_TIE = 1e-9 of a tie (two candidates' centre gaps, the
ego's distance against lateral_reach, the net gap against horizon) is excluded from the comparison
of that car; the excluded share is printed, asserted <= 1 %, and zero in the hand-made frames."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import (COL, DT, TOL, Geo, base_segment, copy_traffic, frame_of, many_car_traffic, move, random_frame,
                       run_lanes4, same_bits, scenes_of, to_np, up)
from world_lib import FollowOracle as Oracle


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in ppamd.FollowCfg._fields_}


def close(got, want, what, keep=None):
    if keep is not None:
        got, want = got[keep], want[keep]
    same = got == want                                  # equal infinities (gap with no leader)
    err = np.abs(np.where(same, 0.0, got - np.where(same, 0.0, want)))
    assert np.all(err <= TOL), (what, float(np.nanmax(err)), int(np.argmax(err)))
    return float(err.max(initial=0.0))


# ---- inputs ---------------------------------------------------------------------------------------
def hand_cases(geo, S):
    """name -> (frame, cfg overrides): the issue's hand-made frames on the longest segment of lane 1
    (cars placed by arc from its start, so a row may lie on a later segment)."""
    s1 = base_segment(geo, 1)[0]
    s0, sL = base_segment(geo, 0)[0], base_segment(geo, geo.NL - 1)[0]
    away = (geo.NL - 1, sL, 5.0, 3.0, 7.0)              # 3 m right of the rightmost lane: in no lane
    n = geo.n
    out = {}
    out["lone"] = (frame_of(geo, S, away, [(1, s1, 10.0, 0.0, 15.0)]), {})
    out["platoon"] = (frame_of(geo, S, away, [(1, s1, 5.0, 0.0, 12.0), (1, s1, 20.0, 0.1, 15.0),
                                              (1, s1, 38.0, -0.2, 10.0)]), {})
    # the follower 6 m before the end of segment n - 1, its leader 9 m into segment 0
    out["wrap"] = (frame_of(geo, S, away, [(0, n - 1, geo.L[0, n - 1] - 6.0, 0.0, 14.0), (0, 0, 9.0, 0.0, 9.0)]), {})
    out["same_arc"] = (frame_of(geo, S, away, [(1, s1, 12.0, -0.3, 10.0), (1, s1, 12.0, 0.3, 12.0)]), {})
    out["parked"] = (frame_of(geo, S, away, [(1, s1, 30.0, 0.0, 0.0), (1, s1, 5.0, 0.0, 10.0)]), {})
    ego_in = (1, s1, 30.0, 0.0, 10.0)
    out["ego_in_lane"] = (frame_of(geo, S, ego_in, [(1, s1, 5.0, 0.0, 15.0), (0, s1, 5.0, 0.0, 15.0)]), {})
    out["ego_between"] = (frame_of(geo, S, (0, s0, 30.0, 2.0, 6.0),
                                   [(0, s0, 5.0, 0.0, 15.0), (1, s0, 6.0, 0.0, 14.0), (2, s0, 7.0, 0.0, 13.0)]),
                          {"lateral_reach": 2.5})
    out["ego_out_of_reach"] = (frame_of(geo, S, away, [(geo.NL - 1, sL, 1.0, 0.0, 15.0)]), {})
    out["ignore_ego"] = (frame_of(geo, S, ego_in, [(1, s1, 5.0, 0.0, 15.0)]), {"react_to_ego": 0})
    out["horizon"] = (frame_of(geo, S, away, [(0, s0, 0.0, 0.0, 20.0), (0, s0, 154.49, 0.0, 5.0),
                                              (2, sL, 0.0, 0.0, 20.0), (2, sL, 154.51, 0.0, 5.0)]), {})
    out["overlap"] = (frame_of(geo, S, away, [(1, s1, 10.0, 0.0, 8.0), (1, s1, 12.0, 0.0, 8.0)]), {})
    out["closing"] = (frame_of(geo, S, away, [(1, s1, 5.0, 0.0, 25.0), (1, s1, 17.5, 0.0, 2.0)]), {})
    return out


HAND = ["lone", "platoon", "wrap", "same_arc", "parked", "ego_in_lane", "ego_between", "ego_out_of_reach",
        "ignore_ego", "horizon", "overlap", "closing"]
HAND_CALLS = 3          # the positions stay, the speeds go on: calls 2 and 3 have v < v0 (the free-road term)


def run_lib(m, fr, cfg, calls, consume=3, dev=None, follow=None):
    """`calls` follow updates of one frame's positions: the host twin (dev None) or pp_traffic_follow
    on torch device `dev`. Returns per call (speed, state) as numpy."""
    S = len(fr["ex"])
    tr = copy_traffic(fr["traffic"], dev)
    sc = scenes_of(fr, dev)
    n = tr["lane"].shape[0]
    if follow is None:
        follow = ppamd.alloc_follow(S, n, xp="numpy" if dev is None else "torch", device=dev)
    out = []
    for _ in range(calls):
        ppamd.traffic_follow(m, sc, tr, follow, consume=consume, cfg=cfg, host=dev is None)
        if dev is not None:
            import torch
            torch.cuda.synchronize()
            out.append((tr["speed"].cpu().numpy(), ppamd.follow_to_numpy(follow)))
        else:
            out.append((tr["speed"].copy(), {k: v.copy() for k, v in follow.items()}))
    return out


def run_oracle(geo, fr, cfg, calls, consume=3):
    o = Oracle(geo, cfg)
    tr = copy_traffic(fr["traffic"])
    J = tr["n_cars"]
    out = []
    for _ in range(calls):
        lead, gap, vn, amb = o.frame(fr["ex"], fr["ey"], fr["mph"], tr, consume)
        tr["speed"][:J] = vn
        out.append((lead, gap, vn, amb))
    return out, o


def compare(got, want, o, J, hand=False):
    """The library's calls against the oracle's under the module docstring's rules. A car that was
    ambiguous in one call is left out of the later calls too (its speed may differ from there on);
    so is every car of its scene, whose leaders' speeds it may have changed."""
    worst = 0.0
    S = got[0][0].shape[1]
    ok = np.ones((J, S), bool)
    for (speed, st), (lead, gap, vn, amb) in zip(got, want):
        ok &= ~amb.any(axis=0)[None]
        np.testing.assert_array_equal(st["leader"][:J][ok], lead[ok])
        worst = max(worst, close(st["gap"][:J], gap, "gap", ok), close(speed[:J], vn, "speed", ok),
                    close(st["desired"][:J], o.desired, "desired"))
        assert (st["started"] == 1).all() and ((st["ego_seg"] >= 1) & (st["ego_seg"] <= o.g.n)).all()
    share = o.excluded / max(o.cars, 1)
    print(f"follow vs oracle: {len(got)} calls x {J} cars x {S} scenes, max |d| {worst:.2e}, near-tie cars "
          f"{o.excluded} ({100 * share:.3f} %)")
    assert share <= 0.01, share
    if hand:
        assert o.excluded == 0
    return worst


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    return {"m": m, "wx": wx, "wy": wy, "geo": Geo(m.geometry())}


# ---- CPU: the host twin against the oracle ---------------------------------------------------------
@pytest.fixture(scope="module")
def hand(cpu):
    S = 5
    out = {}
    for k, (fr, over) in hand_cases(cpu["geo"], S).items():
        cfg = ppamd.default_follow_cfg(**over)
        out[k] = (fr, cfg, run_lib(cpu["m"], fr, cfg, HAND_CALLS), run_oracle(cpu["geo"], fr, cfg, HAND_CALLS))
    assert sorted(out) == sorted(HAND)
    return out


@pytest.mark.parametrize("name", HAND)
def test_hand_made_frames_vs_oracle(hand, name):
    fr, _, got, (want, o) = hand[name]
    compare(got, want, o, fr["traffic"]["n_cars"], hand=True)


def test_hand_made_expectations(hand):
    """The first call of every hand-made frame against figures worked out from its inputs (scene 0)."""
    first = lambda k: (hand[k][2][0][0][:, 0], hand[k][2][0][1]["leader"][:, 0], hand[k][2][0][1]["gap"][:, 0])
    c = cfg_dict(ppamd.default_follow_cfg())
    dt, sab2 = 3 * DT, 2 * np.sqrt(c["max_acc"] * c["comfort_brake"])

    def idm(v, vl, g):          # a car at its desired speed: free = 0
        sstar = c["min_gap"] + max(0.0, v * c["time_headway"] + v * (v - vl) / sab2)
        return v + max(-c["max_acc"] * (sstar / max(g, c["gap_floor"])) ** 2, -c["max_brake"]) * dt

    v, lead, gap = first("lone")
    assert lead[0] == -1 and np.isinf(gap[0]) and v[0] == 15.0
    v, lead, gap = first("platoon")
    assert list(lead) == [1, 2, -1] and abs(gap[0] - 10.5) <= TOL and abs(gap[1] - 13.5) <= TOL and np.isinf(gap[2])
    assert abs(v[0] - idm(12.0, 15.0, 10.5)) <= TOL and abs(v[1] - idm(15.0, 10.0, 13.5)) <= TOL and v[2] == 10.0
    v, lead, gap = first("wrap")
    assert list(lead) == [1, -1] and abs(gap[0] - 10.5) <= TOL and abs(v[0] - idm(14.0, 9.0, 10.5)) <= TOL
    v, lead, gap = first("same_arc")        # car 0 sees car 1 a whole ring ahead; car 1 sees car 0 at gc = 0
    assert list(lead) == [-1, 0] and gap[1] == -4.5 and v[0] == 10.0 and abs(v[1] - (12.0 - 8.0 * dt)) <= TOL
    v, lead, gap = first("parked")
    assert list(lead) == [-1, 0] and v[0] == 0.0 and abs(gap[1] - 20.5) <= TOL and abs(v[1] - idm(10.0, 0.0, 20.5)) <= TOL
    v, lead, gap = first("ego_in_lane")     # n_cars = 2 marks the ego; lane 0's car does not see it
    assert list(lead) == [2, -1] and abs(gap[0] - 20.5) <= TOL and abs(v[0] - idm(15.0, 10.0, 20.5)) <= TOL
    assert v[1] == 15.0
    v, lead, gap = first("ego_between")
    assert list(lead) == [3, 3, -1] and v[0] < 15.0 and v[1] < 14.0 and v[2] == 13.0
    v, lead, gap = first("ego_out_of_reach")
    assert lead[0] == -1 and v[0] == 15.0
    v, lead, gap = first("ignore_ego")
    assert lead[0] == -1 and v[0] == 15.0
    v, lead, gap = first("horizon")
    assert list(lead) == [1, -1, -1, -1] and abs(gap[0] - 149.99) <= TOL and np.isinf(gap[2]) and v[2] == 20.0
    assert v[0] < 20.0
    v, lead, gap = first("overlap")
    assert list(lead) == [1, -1] and abs(gap[0] + 2.5) <= TOL and abs(v[0] - (8.0 - 8.0 * dt)) <= TOL
    v, lead, gap = first("closing")
    assert list(lead) == [1, -1] and abs(gap[0] - 8.0) <= TOL and abs(v[0] - (25.0 - 8.0 * dt)) <= TOL
    # the later calls: below the desired speed the free-road term pulls up again
    v3 = hand["lone"][2][2][0][:, 0]
    assert v3[0] == 15.0
    assert hand["platoon"][2][2][0][2, 0] == 10.0


@pytest.mark.parametrize("n_cars", [0, 1, 12, 100])
@pytest.mark.parametrize("consume", [1, 3, 7])
def test_random_frames_vs_oracle(cpu, n_cars, consume):
    geo = cpu["geo"]
    fr = random_frame(geo, 40, n_cars, 1000 + 10 * n_cars + consume)
    cfg = ppamd.default_follow_cfg()
    got = run_lib(cpu["m"], fr, cfg, 2, consume)
    want, o = run_oracle(geo, fr, cfg, 2, consume)
    compare(got, want, o, n_cars)
    if n_cars >= 12:
        lead = got[0][1]["leader"][:n_cars]
        assert (lead == n_cars).any() and (lead == -1).any() and ((lead >= 0) & (lead < n_cars)).any()


# ---- exact properties -------------------------------------------------------------------------------
def test_free_traffic_keeps_its_speed_bit_for_bit(cpu):
    """Every gap above the horizon and the ego out of reach: ten frames leave the speeds' bits alone."""
    geo, S = cpu["geo"], 7
    s1 = base_segment(geo, 1)[0]
    rows = [(j % geo.NL, s1, 200.0 * (j // geo.NL), 0.1, 5.0 + 1.37 * j) for j in range(12)]
    fr = frame_of(geo, S, (geo.NL - 1, s1, 5.0, 3.0, 7.0), rows)
    tr, sc = copy_traffic(fr["traffic"]), scenes_of(fr)
    follow = ppamd.alloc_follow(S, 12)
    for _ in range(10):
        ppamd.traffic_follow(cpu["m"], sc, tr, follow, consume=3)
        move(geo, tr, 3)
    assert tr["speed"].tobytes() == fr["traffic"]["speed"].tobytes()
    assert (follow["leader"] == -1).all() and np.isinf(follow["gap"]).all()


def episode(cpu, fr, F, consume, fresh_arrays, follow=None):
    """F frames of follow + move on the host. fresh_arrays: every call gets newly allocated copies of
    the traffic and the state (nothing of an episode lives outside the caller's arrays)."""
    tr, sc = copy_traffic(fr["traffic"]), scenes_of(fr)
    follow = follow if follow is not None else ppamd.alloc_follow(len(fr["ex"]), tr["lane"].shape[0])
    for _ in range(F):
        if fresh_arrays:
            tr, follow = copy_traffic(tr), {k: v.copy() for k, v in follow.items()}
        ppamd.traffic_follow(cpu["m"], sc, tr, follow, consume=consume)
        move(cpu["geo"], tr, consume)
    return tr, follow


def test_calls_of_one_frame_equal_one_episode(cpu):
    """F calls of one frame, each on fresh copies of the arrays of the call before, equal the F-frame
    episode on one set of arrays bit for bit: the state arrays carry everything."""
    fr = random_frame(cpu["geo"], 9, 12, 77)
    a, fa = episode(cpu, fr, 25, 3, False)
    b, fb = episode(cpu, fr, 25, 3, True)
    same_bits({k: v for k, v in a.items() if k != "n_cars"}, {k: v for k, v in b.items() if k != "n_cars"}, "traffic")
    same_bits(fa, fb, "state")
    assert (fa["leader"] >= 0).any() and (a["speed"] != fr["traffic"]["speed"]).any()


def test_reused_state_restarts_from_zero_started(cpu):
    fr, other = random_frame(cpu["geo"], 9, 12, 78), random_frame(cpu["geo"], 9, 12, 79)
    _, used = episode(cpu, other, 5, 3, False)
    used["started"][:] = 0
    a, fa = episode(cpu, fr, 5, 3, False, follow=used)
    b, fb = episode(cpu, fr, 5, 3, False)
    assert a["speed"].tobytes() == b["speed"].tobytes()
    same_bits(fa, fb, "state")


# ---- the point of the feature -----------------------------------------------------------------------
GAPS = [12.0, 16.0, 20.0, 25.0, 30.0, 40.0, 50.0]
CAR_V = 15.0


def rear_end_start(cpu):
    """One scene per start gap: the ego of synthetic scene 0 at rest with no previous path, and one
    car GAPS[s] metres (centre to centre) behind it in its lane at 15 m/s."""
    geo, S = cpu["geo"], len(GAPS)
    sc0, _ = ppamd.synth_traffic_host(cpu["m"], 1, seed=23)
    sc = ppamd.add_car_table(ppamd.alloc_scenes(S, 12))
    for k in ("ego_x", "ego_y", "ego_yaw_deg"):
        sc[k][:] = sc0[k][0]
    o = Oracle(geo, ppamd.default_follow_cfg())
    arc_e, dist_e = o.ego_on_lanes(np.stack([sc["ego_x"], sc["ego_y"]], -1))
    lane = int(dist_e[:, 0].argmin())
    assert dist_e[lane, 0] < 0.5
    sc["prev_target_lane"][:] = lane
    tr = ppamd.alloc_traffic(S, n=1)
    sg, t = geo.place(np.full(S, lane), np.zeros(S, int), np.zeros(S), arc_e[lane] - np.array(GAPS))
    tr["lane"][0], tr["seg"][0], tr["t"][0], tr["speed"][0] = lane, sg, t, CAR_V
    tr["n_cars"] = 1
    return sc, tr


def drive(cpu, sc, tr, F, follow_on):
    """oracle_rollout one frame at a time, the host judge on every frame; with follow_on,
    traffic_follow(host) before each frame. Returns the judge state and the car's speed per frame."""
    olib = oracle_lib.load_oracle()
    sc, tr = oracle_lib.copy_state(sc, tr)
    S = len(sc["ego_x"])
    prm = ppamd.default_params(n_speeds=1)
    judge, follow = ppamd.alloc_judge(S), ppamd.alloc_follow(S, 1)
    speeds = []
    for _ in range(F):
        if follow_on:
            ppamd.traffic_follow(cpu["m"], sc, tr, follow, consume=3)
        speeds.append(tr["speed"][0].copy())
        pre_sc, pre_tr = oracle_lib.copy_state(sc, tr)
        lg = oracle_lib.oracle_rollout(olib, cpu["wx"], cpu["wy"], sc, tr, prm, 1, 3, 400.0)
        res = {"n_out": np.ascontiguousarray(lg["n_out"][0]), "next_x": np.ascontiguousarray(lg["plan_x"][0]),
               "next_y": np.ascontiguousarray(lg["plan_y"][0])}
        ppamd.judge_frame(cpu["m"], pre_sc, pre_tr, res, judge, consume=3)
    return ppamd.judge_to_numpy(judge), np.array(speeds)


def test_follower_does_not_rear_end_an_ego_pulling_away(cpu):
    """The constant-speed car runs the ego over from behind; the same start with following on does
    not, and the follower's speed dips below its desired speed and rises again behind the ego."""
    sc, tr = rear_end_start(cpu)
    F = 300
    ghost, _ = drive(cpu, sc, tr, F, False)
    hit = (ghost["flags"] & ppamd.INC_COLLISION) != 0
    print("constant speed: collided", dict(zip(GAPS, hit.tolist())), "min_sep", ghost["min_sep"].round(2).tolist())
    assert hit.any(), "no start gap at which the constant-speed car collides"
    s = int(np.nonzero(hit)[0].max())                   # the widest gap that still collides
    assert ghost["first_car"][s] == 1
    got, v = drive(cpu, sc, tr, F, True)
    print("following:      collided", dict(zip(GAPS, ((got["flags"] & ppamd.INC_COLLISION) != 0).tolist())),
          "min_sep", got["min_sep"].round(2).tolist(), f"; gap {GAPS[s]} m: slowest {v[:, s].min():.2f} m/s at frame "
          f"{int(v[:, s].argmin())}, last {v[-1, s]:.2f} m/s")
    assert not got["flags"][s] & ppamd.INC_COLLISION and got["count"][COL, s] == 0 and got["min_sep"][s] > 0
    k = int(v[:, s].argmin())
    assert v[k, s] < CAR_V - 1.0 and v[-1, s] > v[k, s] + 1.0 and k < F - 1
    # a gap from which the model has room to stop (the issue's bound) must never collide
    c = cfg_dict(ppamd.default_follow_cfg())
    safe = CAR_V ** 2 / (2 * c["comfort_brake"]) + CAR_V * c["time_headway"] + c["min_gap"] + c["car_length"]
    for i, g in enumerate(GAPS):
        if g >= safe:
            assert not got["flags"][i] & ppamd.INC_COLLISION, g


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors(cpu):
    geo = cpu["geo"]
    fr = hand_cases(geo, 2)["platoon"][0]
    sc = ppamd.add_car_table(scenes_of(fr))
    b, T = ppamd.scene_struct(sc), ppamd.traffic_struct(fr["traffic"])
    follow = ppamd.alloc_follow(2, 3)
    Fs = ppamd.follow_struct(follow)
    prm = ppamd.default_params(n_speeds=1)
    res = ppamd.alloc_result(2, prm)
    R = ppamd.result_struct(res)
    rc = ppamd.RolloutCfg(1, 3, 100.0)
    before = fr["traffic"]["speed"].copy()

    def call(cfg, consume=3, state=Fs, host=True, scenes=b):
        st = C.byref(state) if state is not None else None
        if host:
            return ppamd.lib.pp_traffic_follow_host(cpu["m"].handle, C.byref(scenes), C.byref(T), consume,
                                                    C.byref(cfg) if cfg is not None else None, st)
        return ppamd.lib.pp_traffic_follow(cpu["m"].handle, C.byref(scenes), C.byref(T), consume,
                                           C.byref(cfg) if cfg is not None else None, st, 0, None)

    def reactive(cfg, state=Fs, jcfg=None, jstate=None):
        return ppamd.lib.pp_rollout_reactive(cpu["m"].handle, C.byref(b), C.byref(T), C.byref(prm), C.byref(rc),
                                             C.byref(R), None, 0, None, jcfg, jstate,
                                             C.byref(cfg) if cfg is not None else None,
                                             C.byref(state) if state is not None else None)

    ok = ppamd.default_follow_cfg()
    assert [getattr(ok, k) for k, _ in ppamd.FollowCfg._fields_[:-1]] == \
        [2.0, 3.0, 8.0, 1.2, 2.0, 0.5, 150.0, 4.5, 4.5, 2.0, 1]
    bad = [{"max_acc": 0.0}, {"max_acc": -1.0}, {"comfort_brake": 0.0}, {"max_brake": 0.0}, {"max_brake": -8.0},
           {"gap_floor": 0.0}, {"car_length": -0.1}, {"ego_length": -0.1}, {"lateral_reach": -1.0},
           {"horizon": -1.0}, {"max_acc": float("nan")}, {"horizon": float("nan")}]
    for host in (True, False):       # every check comes before any HIP call
        for over in bad:
            assert call(ppamd.default_follow_cfg(**over), host=host) == -1, over
        assert call(None, host=host) == -1
        assert call(ok, state=None, host=host) == -1
        assert call(ok, consume=0, host=host) == -1
        for hole in ("started", "ego_seg", "desired", "next_speed", "leader", "gap"):
            holed = ppamd.follow_struct(follow)
            setattr(holed, hole, None)
            assert call(ok, state=holed, host=host) == -1, hole
        nospeed = ppamd.scene_struct(sc)
        nospeed.ego_speed_mph = None
        assert call(ok, scenes=nospeed, host=host) == -1
    for over in bad:
        assert reactive(ppamd.default_follow_cfg(**over)) == -1, over
    assert reactive(None) == -1 and reactive(ok, state=None) == -1
    holed = ppamd.follow_struct(follow)
    holed.next_speed = None
    assert reactive(ok, state=holed) == -1
    J = ppamd.judge_struct(ppamd.alloc_judge(2))
    assert reactive(ok, jcfg=None, jstate=C.byref(J)) == -1                 # a judge state wants its configuration
    badj = ppamd.default_judge_cfg(acc_window=0)
    assert reactive(ok, jcfg=C.byref(badj), jstate=C.byref(J)) == -1
    assert not follow["started"].any() and fr["traffic"]["speed"].tobytes() == before.tobytes()
    zero = ppamd.default_follow_cfg(horizon=0.0, car_length=0.0, ego_length=0.0, lateral_reach=0.0)
    assert call(zero) == 0                                                 # zero is allowed where negative is not


# ---- the four-lane build ------------------------------------------------------------------------------
def test_four_lane_build_host():
    """The 4-lane library follows an ego and a car on lane 3 (tests/follow_lanes4_cases.py, a child
    process: a process loads one PP_NUM_LANES)."""
    run_lanes4("follow_lanes4_cases.py", "not gpu")


# ---- GPU ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
class TestFollowGPU:
    @pytest.fixture(scope="class")
    def env(self, cpu):
        import torch
        return dict(cpu, torch=torch, dev=torch.device("cuda", 0))

    def same_calls(self, a, b, what):
        for i, ((va, sa), (vb, sb)) in enumerate(zip(a, b)):
            assert va.tobytes() == vb.tobytes(), f"{what} call {i} speed"
            same_bits(sa, sb, f"{what} call {i}")

    @pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
    def test_device_equals_host_twin_bit_for_bit(self, env, S):
        """The hand-made frames (1 to 4 cars) and random frames of 0, 1, 12 and 100 cars."""
        for name, (fr, over) in hand_cases(env["geo"], S).items():
            cfg = ppamd.default_follow_cfg(**over)
            self.same_calls(run_lib(env["m"], fr, cfg, HAND_CALLS, dev=env["dev"]),
                            run_lib(env["m"], fr, cfg, HAND_CALLS), name)
        cfg = ppamd.default_follow_cfg()
        for n_cars, consume in ((0, 3), (1, 1), (12, 3), (100, 7)):
            fr = random_frame(env["geo"], S, n_cars, 5000 + n_cars)
            self.same_calls(run_lib(env["m"], fr, cfg, 2, consume, dev=env["dev"]),
                            run_lib(env["m"], fr, cfg, 2, consume), f"random {n_cars}")

    def test_dense_traffic_device_equals_host_frame_by_frame(self, env):
        """Dense 100-car traffic, 64 scenes x 150 frames of pp_rollout_reactive (judge on), one frame per
        call; the host twins recompute follow and judge from the GPU's own pre-frame state: every
        field of both states bit for bit. Fewer scenes collide than in the same drive under
        pp_rollout_judged."""
        t, dev = env["torch"], env["dev"]
        S, F, n = 64, 150, 100
        sc, tr = many_car_traffic(env["m"], S, 23, dense=True)
        prm = ppamd.default_params(n_speeds=1)
        jcfg, fcfg = ppamd.default_judge_cfg(), ppamd.default_follow_cfg()
        d = {k: up(v, dev) for k, v in sc.items()}
        g = {k: up(v, dev) for k, v in tr.items()}
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        plain = ppamd.alloc_judge(S, xp="torch", device=dev)
        ppamd.rollout_judged(env["m"], d, g, prm, res, plain, F, 3, 400.0, cfg=jcfg)
        t.cuda.synchronize()
        ghost = ppamd.judge_to_numpy(plain)
        ppamd.plan_reset(env["m"])
        d = {k: up(v, dev) for k, v in sc.items()}
        g = {k: up(v, dev) for k, v in tr.items()}
        follow = ppamd.alloc_follow(S, n, xp="torch", device=dev)
        hj, hf = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n)
        for f in range(F):
            pre_sc, pre_tr = to_np(d), to_np(g)
            ppamd.rollout_reactive(env["m"], d, g, prm, res, follow, 1, 3, 400.0, judge=judge, jcfg=jcfg, fcfg=fcfg)
            t.cuda.synchronize()
            ppamd.traffic_follow(env["m"], pre_sc, pre_tr, hf, consume=3, cfg=fcfg)
            assert pre_tr["speed"].tobytes() == g["speed"].cpu().numpy().tobytes(), f"frame {f} speed"
            same_bits(ppamd.follow_to_numpy(follow), hf, f"frame {f} follow")
            plan = {k: res[k].cpu().numpy() for k in ("n_out", "next_x", "next_y")}
            ppamd.judge_frame(env["m"], pre_sc, pre_tr, plan, hj, consume=3, cfg=jcfg)
        got = ppamd.judge_to_numpy(judge)
        same_bits(got, ppamd.judge_to_numpy(hj), "dense judge")
        n_ghost = int(((ghost["flags"] & ppamd.INC_COLLISION) != 0).sum())
        n_react = int(((got["flags"] & ppamd.INC_COLLISION) != 0).sum())
        print(f"dense 100 cars, {S} scenes x {F} frames: {n_ghost} scenes collide at constant speed, {n_react} with "
              f"following")
        assert n_react < n_ghost

    def start(self, env, S, seed=11):
        t = env["torch"]
        d, g = ppamd.synth_traffic(env["m"], S, seed=seed, device=0)
        t.cuda.synchronize()
        return d, g

    def test_one_call_equals_one_frame_calls(self, env):
        """One 40-frame call equals 40 one-frame calls, bit for bit (S = 384)."""
        t, dev = env["torch"], env["dev"]
        S, F = 384, 40
        prm = ppamd.default_params(n_speeds=1)
        runs = []
        for calls in (1, F):
            ppamd.plan_reset(env["m"])
            d, g = self.start(env, S)
            res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
            lg = ppamd.alloc_log(F, S, 50, xp="torch", device=dev)
            judge = ppamd.alloc_judge(S, xp="torch", device=dev)
            follow = ppamd.alloc_follow(S, 12, xp="torch", device=dev)
            for c in range(calls):
                part = lg if calls == 1 else {k: v[c:c + 1] for k, v in lg.items()}
                ppamd.rollout_reactive(env["m"], d, g, prm, res, follow, F // calls, 3, 100.0, part, judge=judge)
            t.cuda.synchronize()
            runs.append([to_np(x) for x in (d, {k: v for k, v in g.items() if k != "n_cars"}, res, lg, follow)] +
                        [ppamd.judge_to_numpy(judge)])
        for what, a, b in zip(("scenes", "traffic", "result", "log", "follow", "judge"), *runs):
            same_bits({k: v for k, v in a.items() if v is not None}, {k: v for k, v in b.items() if v is not None}, what)
        assert (runs[0][4]["leader"] >= 0).any()

    def test_free_traffic_rollout_reactive_equals_rollout(self, env):
        """Far-apart traffic with the ego out of reach (react_to_ego stays 1: the cars start half a loop
        from the ego, 200 m apart per lane): scenes, traffic, result and log equal pp_rollout's bit
        for bit."""
        t, dev = env["torch"], env["dev"]
        S, F = 130, 20
        geo = env["geo"]
        prm = ppamd.default_params(n_speeds=1)
        runs = []
        for reactive in (False, True):
            ppamd.plan_reset(env["m"])
            d, g = self.start(env, S, seed=12)
            ego = np.stack([d["ego_x"].cpu().numpy(), d["ego_y"].cpu().numpy()], -1)
            arc_e = Oracle(geo, ppamd.default_follow_cfg()).ego_on_lanes(ego)[0]
            for j in range(12):                          # lane j % NL, 200 m apart, from half a loop ahead of the ego
                lane = np.full(S, j % geo.NL)
                sg, tt = geo.place(lane, np.zeros(S, int), np.zeros(S),
                                   arc_e[j % geo.NL] + geo.tot[j % geo.NL] / 2 + 200.0 * (j // geo.NL))
                g["lane"][j], g["seg"][j], g["t"][j] = up(lane.astype(np.int32), dev), up(sg.astype(np.int32), dev), up(tt, dev)
            d["n_cars"][:] = 0
            res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
            lg = ppamd.alloc_log(F, S, 50, xp="torch", device=dev)
            follow = ppamd.alloc_follow(S, 12, xp="torch", device=dev)
            if reactive:
                ppamd.rollout_reactive(env["m"], d, g, prm, res, follow, F, 3, 100.0, lg)
            else:
                ppamd.rollout(env["m"], d, g, prm, res, F, 3, 100.0, lg)
            t.cuda.synchronize()
            runs.append([to_np(x) for x in (d, {k: v for k, v in g.items() if k != "n_cars"}, res, lg, follow)])
        for what, a, b in zip(("scenes", "traffic", "result", "log"), *runs):
            same_bits({k: v for k, v in a.items() if v is not None}, {k: v for k, v in b.items() if v is not None}, what)
        assert (runs[1][4]["leader"] == -1).all() and (runs[1][4]["started"] == 1).all()

    def test_four_lane_build_device(self):
        run_lanes4("follow_lanes4_cases.py", "gpu")
