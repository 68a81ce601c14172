"""Lane-changing traffic (include/pp.h pp_traffic_lane_change, pp_rollout_lane_changing;
csrc/pp_lanechange.h): after the follow update of a frame, a traffic car moves to a neighbour lane when
MOBIL says so; at most one car per scene begins a change per call.

The definitions are the project's own (DESIGN.md "Lane-changing traffic"); the reference has no
simulator, so nothing here is compared with it. The oracle is the NumPy restatement below, written
from those definitions and not from the header: the car is projected on EVERY segment of the target
lane (no window around its own segment), the new leader and the new follower are argmins over full
[car, candidate] gap matrices, the accelerations are one vectorised expression. The oracle reads
what the call reads: the pre-call traffic and lane-change state, and the follow state the library's
(separately tested) follow update left.

Tolerances. `lane`, `seg`, `dir`, `last_car`, `last_dir`, `wait`, `changes`, `n_changes` are exact.
`t`, `offset`, `arc`, `gain` within TOL = 1e-8 (test_judge's): a gain is a handful of roundings of
magnitudes <= 10 m/s^2. A scene whose ORACLE decision lies within TIE = 1e-9 of a tie (two surpluses,
a surplus against 0, a safety bound, two candidates' gaps, the horizon, lateral_reach, the lateral
step, the two nearest segment distances of the winner's projection) is left out of the comparison;
two surpluses that are equal to the bit (a car with both neighbour lanes empty) are no near-tie: the
tie rule decides them. The left-out share is printed, asserted <= 1 % on the random frames and 0 on
the hand-made frames."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib
import world_lib as wl
from oracle_lib import ppamd
from world_lib import (DT, MPH, TOL, Geo, base_segment, frame_of, many_car_traffic, run_lanes4, same_bits, to_np,
                       up)

TIE = 1e-9
INF = float("inf")
INT_KEYS = ("started", "n_changes", "last_car", "last_dir", "wait", "changes", "dir")
TR_KEYS = ("lane", "seg", "t", "offset", "speed")


def fdict(cfg):
    return {k: getattr(cfg, k) for k, _ in ppamd.FollowCfg._fields_}


def ldict(cfg):
    return {k: getattr(cfg, k) for k, _ in ppamd.LaneChangeCfg._fields_}


# ---- the oracle -----------------------------------------------------------------------------------
def idm(F, v, v0, lead, vl, g):
    """The acceleration of the follow model, vectorised (v0 <= 0 gives a number nobody uses)."""
    with np.errstate(all="ignore"):
        r = v / np.where(v0 > 0, v0, 1.0)
        free = 1 - r ** 4
        dyn = v * F["time_headway"] + v * (v - vl) / (2 * np.sqrt(F["max_acc"] * F["comfort_brake"]))
        q = (F["min_gap"] + np.maximum(dyn, 0.0)) / np.maximum(g, F["gap_floor"])
        a = F["max_acc"] * np.where(lead, free - q ** 2, free)
    return np.maximum(a, -F["max_brake"])


def pick(a, i):
    """a[i[j, s], s] for a [J, S], any i (clipped)."""
    return np.take_along_axis(a, np.clip(i, 0, a.shape[0] - 1), 0)


def nearest(mat):
    """Column of the first minimum of [J, K, S] along K, the minimum, and whether a second is within TIE."""
    col = mat.argmin(1)
    srt = np.sort(mat, axis=1)
    first = srt[:, 0]
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(first) & (srt[:, 1] - np.where(np.isfinite(first), first, 0.0) <= TIE)
    return col, first, tie


def oracle_call(geo, fcfg, lcfg, sc, tr, fo, lc, consume):
    """One call over S scenes: returns (traffic, state) after it and the near-tie scenes [S]."""
    F, c = fdict(fcfg), ldict(lcfg)
    ex, ey, mph = sc["ego_x"], sc["ego_y"], sc["ego_speed_mph"]
    J, S = int(tr["n_cars"]), len(ex)
    pre_tr, pre_lc = tr, lc
    tr = wl.copy_traffic(tr)
    lc = {k: v.copy() for k, v in lc.items()}
    amb = np.zeros(S, bool)
    if J == 0:
        return tr, lc, amb
    act = fo["started"] != 0
    lane, seg, t, v = tr["lane"][:J], tr["seg"][:J], tr["t"][:J], tr["speed"][:J]
    fresh = act & (lc["started"] == 0)
    lc["home"][:J][:, fresh] = tr["offset"][:J][:, fresh]
    lc["wait"][:J][:, fresh] = 0
    lc["changes"][:J][:, fresh] = 0
    lc["n_changes"][fresh] = 0
    lc["started"][act] = 1
    home = lc["home"][:J]
    d = home - tr["offset"][:J]
    step = c["lateral_speed"] * consume * DT
    off = np.where(np.abs(d) <= step, home, tr["offset"][:J] + np.where(d > 0, step, -step))
    amb |= ((d != 0) & (np.abs(np.abs(d) - step) <= TIE)).any(0)
    wait = np.maximum(lc["wait"][:J] - consume, 0)
    transit = off != home
    arc = geo.cum0[lane, seg] + t * geo.L[lane, seg]
    arc_e, dist_e = wl.FollowOracle(geo, fcfg).ego_on_lanes(np.stack([ex, ey], -1))       # [NL, S]
    react = bool(F["react_to_ego"])
    occ = (dist_e <= F["lateral_reach"]) & react
    amb |= ((np.abs(dist_e - F["lateral_reach"]) <= TIE) & react).any(0)
    ve = np.asarray(mph) / MPH
    v0, lead, gap = fo["desired"][:J], fo["leader"][:J], fo["gap"][:J]
    elig = (v0 > 0) & (wait == 0) & ~transit
    s_ix = np.arange(S)[None]
    j_ix, m_ix = np.arange(J)[:, None, None], np.arange(J)[None, :, None]
    with np.errstate(all="ignore"):
        vlead = np.where(lead == J, ve[None], pick(v, lead))
        a_now = idm(F, v, v0, lead >= 0, vlead, gap)
        # the old follower: the lowest car whose recorded leader this car is
        is_old = lead[None, :, :] == j_ix
        has_o, o = is_old.any(1), is_old.argmax(1)
        v_o, v0_o, g_o = pick(v, o), pick(v0, o), pick(gap, o)
        g2 = g_o + gap + F["car_length"]
        counts_o = has_o & (v0_o > 0)
        d_old = np.where(counts_o, idm(F, v_o, v0_o, (lead >= 0) & (g2 <= F["horizon"]), vlead, g2) -
                         idm(F, v_o, v0_o, True, v, g_o), 0.0)
        near_old = counts_o & (lead >= 0) & (np.abs(g2 - F["horizon"]) <= TIE)
    P = geo.car(lane, seg, t, off)[0]                                               # [J, S, 2]
    sur, place = {}, {}
    for dl in (-1, 1):
        l2 = lane + dl
        inr = (l2 >= 0) & (l2 < geo.NL)
        lx = np.clip(l2, 0, geo.NL - 1)
        with np.errstate(all="ignore"):
            # the car on every segment of the target lane
            A_, D_ = geo.A[lx], geo.D[lx]                                           # [J, S, n, 2]
            ap = P[:, :, None, :] - A_
            tt = np.clip((ap * D_).sum(-1) / (D_ ** 2).sum(-1), 0.0, 1.0)
            q = ap - D_ * tt[..., None]
            dist = np.sqrt((q ** 2).sum(-1))                                        # [J, S, n]
            k = dist.argmin(-1)
            srt = np.sort(dist, axis=-1)
            proj_tie = srt[..., 1] - srt[..., 0] <= TIE
            t2 = np.take_along_axis(tt, k[..., None], -1)[..., 0]
            qq = np.take_along_axis(q, k[..., None, None], 2)[:, :, 0]              # P - Q
            u = geo.U[lx, k]
            off2 = qq[..., 0] * u[..., 1] - qq[..., 1] * u[..., 0]
            arc2 = geo.cum0[lx, k] + t2 * geo.L[lx, k]
            loop = geo.tot[lx]
            place[dl] = (k, t2, off2, proj_tie)
            # candidates on the target lane: column 0 the ego, column m + 1 car m (the rank order)
            fwd = np.full((J, J + 1, S), np.inf)
            bwd = np.full((J, J + 1, S), np.inf)
            ce = arc_e[lx, s_ix] - arc2
            fwd[:, 0] = np.where(occ[lx, s_ix], np.where(ce < 0, ce + loop, ce), np.inf)
            ce = arc2 - arc_e[lx, s_ix]
            bwd[:, 0] = np.where(occ[lx, s_ix], np.where(ce <= 0, ce + loop, ce), np.inf)
            on = (lane[None, :, :] == l2[:, None, :]) & (m_ix != j_ix)
            cc = arc[None, :, :] - arc2[:, None, :]
            fwd[:, 1:] = np.where(on, np.where(cc < 0, cc + loop[:, None, :], cc), np.inf)
            cc = arc2[:, None, :] - arc[None, :, :]
            bwd[:, 1:] = np.where(on, np.where(cc <= 0, cc + loop[:, None, :], cc), np.inf)
            # the new leader
            coln, cn, tie_n = nearest(fwd)
            n_ego = coln == 0
            g_n = cn - (F["car_length"] + np.where(n_ego, F["ego_length"], F["car_length"])) / 2
            has_n = np.isfinite(cn) & (g_n <= F["horizon"])
            near = tie_n | (np.isfinite(cn) & (np.abs(g_n - F["horizon"]) <= TIE))
            v_n = np.where(n_ego, ve[None], pick(v, coln - 1))
            a_j2 = idm(F, v, v0, has_n, v_n, np.where(has_n, g_n, np.inf))
            # the new follower
            colf, cf, tie_f = nearest(bwd)
            f_ego = colf == 0
            g_f = cf - (np.where(f_ego, F["ego_length"], F["car_length"]) + F["car_length"]) / 2
            has_f = np.isfinite(cf) & (g_f <= F["horizon"])
            near |= tie_f | (np.isfinite(cf) & (np.abs(g_f - F["horizon"]) <= TIE))
            v_f, v0_f = pick(v, colf - 1), pick(v0, colf - 1)
            parked_f = ~f_ego & ~(v0_f > 0)
            a_f2 = np.where(f_ego, idm(F, np.broadcast_to(ve[None], v.shape), c["ego_desired_speed"], True, v, g_f),
                            np.where(parked_f, 0.0, idm(F, v_f, v0_f, True, v, g_f)))
            d_f = np.where(has_f & ~f_ego & ~parked_f, a_f2 - pick(a_now, colf - 1), 0.0)
            safe = (~has_n | (g_n >= F["min_gap"])) & (~has_f | (g_f >= F["min_gap"])) & \
                (~has_f | (a_f2 >= -c["safe_brake"])) & (a_j2 >= -c["safe_brake"])
            near |= (has_n & (np.abs(g_n - F["min_gap"]) <= TIE)) | (has_f & (np.abs(g_f - F["min_gap"]) <= TIE)) | \
                (has_f & (np.abs(a_f2 + c["safe_brake"]) <= TIE)) | (np.abs(a_j2 + c["safe_brake"]) <= TIE) | near_old
            gain = (a_j2 - a_now) + c["politeness"] * (d_f + d_old)
            s_ = gain - c["threshold"] - (c["right_bias"] if dl < 0 else -c["right_bias"])
        sur[dl] = np.where(elig & inr & safe, s_, -np.inf)
        amb |= (near & elig & inr).any(0)
    s0, s1 = sur[-1], sur[1]
    best = np.maximum(s0, s1)
    dirs = np.where(best > -np.inf, np.where(s1 > s0, 1, -1), 0)
    with np.errstate(invalid="ignore"):
        amb |= (np.isfinite(s0) & np.isfinite(s1) & (s0 != s1) & (np.abs(s1 - s0) <= TIE)).any(0)
        amb |= (np.abs(best) <= TIE).any(0)
        jw = best.argmax(0)
        bw = best[jw, np.arange(S)]
        if J > 1:
            second = np.sort(best, axis=0)[-2]
            amb |= (bw > 0) & (second != bw) & (bw - second <= TIE)
    wins = (bw > 0) & act
    lc["last_car"][act], lc["last_dir"][act] = 0, 0
    for s in np.nonzero(wins)[0]:
        j = jw[s]
        dl = int(dirs[j, s])
        k, t2, off2, proj_tie = place[dl]
        amb[s] |= proj_tie[j, s]
        lane[j, s], seg[j, s], t[j, s], off[j, s] = lane[j, s] + dl, k[j, s], t2[j, s], off2[j, s]
        wait[j, s] = c["min_interval_steps"]
        lc["changes"][j, s] += 1
        lc["n_changes"][s] += 1
        lc["last_car"][s], lc["last_dir"][s] = j + 1, dl
    tr["offset"][:J] = off
    lc["wait"][:J], lc["arc"][:J], lc["gain"][:J], lc["dir"][:J] = wait, arc, best, dirs
    for k_ in TR_KEYS:                                   # a scene the follow update has not started is left alone
        tr[k_][:, ~act] = pre_tr[k_][:, ~act]
    for k_, a in lc.items():
        a[..., ~act] = pre_lc[k_][..., ~act]
    return tr, lc, amb & act


def close(got, want, what, keep):
    got, want = got[..., keep], want[..., keep]
    same = got == want                                   # equal infinities
    with np.errstate(invalid="ignore"):
        err = np.abs(np.where(same, 0.0, got - np.where(same, 0.0, want)))
    assert np.all(err <= TOL), (what, float(np.nanmax(err)), int(np.argmax(err)))
    return float(err.max(initial=0.0))


class Tally:
    def __init__(self):
        self.scenes = self.left_out = 0
        self.worst = 0.0

    def check(self, got_tr, got_lc, want_tr, want_lc, amb, J):
        keep = ~amb
        self.scenes += len(amb)
        self.left_out += int(amb.sum())
        for k in ("lane", "seg"):
            np.testing.assert_array_equal(got_tr[k][:J][:, keep], want_tr[k][:J][:, keep], err_msg=k)
        assert got_tr["speed"].tobytes() == want_tr["speed"].tobytes()
        for k in INT_KEYS:
            np.testing.assert_array_equal(got_lc[k][..., keep], want_lc[k][..., keep], err_msg=k)
        np.testing.assert_array_equal(got_lc["home"][:J][:, keep], want_lc["home"][:J][:, keep])
        self.worst = max(self.worst, close(got_tr["t"][:J], want_tr["t"][:J], "t", keep),
                         close(got_tr["offset"][:J], want_tr["offset"][:J], "offset", keep),
                         close(got_lc["arc"][:J], want_lc["arc"][:J], "arc", keep),
                         close(got_lc["gain"][:J], want_lc["gain"][:J], "gain", keep))

    def done(self, what, hand=False):
        share = self.left_out / max(self.scenes, 1)
        print(f"lane change vs oracle, {what}: {self.scenes} scene calls, max |d| {self.worst:.2e}, near-tie scenes "
              f"{self.left_out} ({100 * share:.3f} %)")
        assert share <= 0.01, share
        if hand:
            assert self.left_out == 0


# ---- worlds: scenes, traffic, follow state, lane-change state ---------------------------------------
def world(sc, tr, dev=None):
    S, n = len(sc["ego_x"]), tr["lane"].shape[0]
    xp = "numpy" if dev is None else "torch"
    w = {"sc": {k: np.array(v, copy=True) for k, v in sc.items()}, "tr": wl.copy_traffic(tr)}
    if dev is not None:
        w["sc"] = {k: up(v, dev) for k, v in w["sc"].items()}
        w["tr"] = {k: up(v, dev) for k, v in w["tr"].items()}
    w["fo"] = ppamd.alloc_follow(S, n, xp=xp, device=dev)
    w["lc"] = ppamd.alloc_lane_change(S, n, xp=xp, device=dev)
    return w


def frame_world(fr, dev=None):
    return world(wl.scenes_of(fr), fr["traffic"], dev)


def snap(w):
    return {k: to_np(w[k]) for k in ("sc", "tr", "fo", "lc")}


def follow_then_change(m, w, consume=3, fcfg=None, lcfg=None, geo=None, tally=None):
    """One frame's follow update and lane changes on the world's own arrays (host or device). With a
    tally (host worlds), the lane-change call is checked against the oracle from its own inputs."""
    host = isinstance(w["sc"]["ego_x"], np.ndarray)
    fcfg = fcfg if fcfg is not None else ppamd.default_follow_cfg()
    lcfg = lcfg if lcfg is not None else ppamd.default_lane_change_cfg()
    ppamd.traffic_follow(m, w["sc"], w["tr"], w["fo"], consume=consume, cfg=fcfg, host=host)
    if tally is not None:
        want_tr, want_lc, amb = oracle_call(geo, fcfg, lcfg, w["sc"], w["tr"], w["fo"], w["lc"], consume)
    fo_before = {k: v.copy() for k, v in w["fo"].items()} if host else None
    ppamd.traffic_lane_change(m, w["sc"], w["tr"], w["fo"], w["lc"], consume=consume, fcfg=fcfg, cfg=lcfg, host=host)
    if host:
        same_bits(w["fo"], fo_before, "the follow state is read only")
    if tally is not None:
        tally.check(w["tr"], w["lc"], want_tr, want_lc, amb, int(w["tr"]["n_cars"]))


def move(geo, tr, consume):
    wl.move(geo, tr, consume)


# ---- hand-made frames --------------------------------------------------------------------------------
FAST, SLOW = 20.0, 10.0


def overtake_rows(geo, lane=1, extra=()):
    """A 20 m/s car 40 m behind a 10 m/s car on `lane` (from 15 m into lane 1's longest segment)."""
    s1 = base_segment(geo, 1)[0]
    return [(lane, s1, 15.0, 0.0, FAST), (lane, s1, 55.0, 0.0, SLOW)] + [tuple(r) for r in extra], s1


def away(geo):
    sL = base_segment(geo, geo.NL - 1)[0]
    return (geo.NL - 1, sL, 5.0, 3.0, 7.0)               # 3 m right of the rightmost lane: in no lane


def overtake(geo, S=5, lane=1, extra=(), ego=None):
    rows, _ = overtake_rows(geo, lane, extra)
    return frame_of(geo, S, ego if ego is not None else away(geo), rows)


def sidm(F, v, v0, vl=None, g=None):
    """Scalar IDM, worked out in the test."""
    free = 1 - (v / v0) ** 4
    a = F["max_acc"] * free
    if vl is not None:
        sstar = F["min_gap"] + max(0.0, v * F["time_headway"] + v * (v - vl) / (2 * math.sqrt(F["max_acc"] * F["comfort_brake"])))
        a = F["max_acc"] * (free - (sstar / max(g, F["gap_floor"])) ** 2)
    return max(a, -F["max_brake"])


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    return {"m": m, "wx": wx, "wy": wy, "geo": Geo(m.geometry())}


def first_call(cpu, fr, fover=None, lover=None, tally=None):
    w = frame_world(fr)
    follow_then_change(cpu["m"], w, 3, ppamd.default_follow_cfg(**(fover or {})),
                       ppamd.default_lane_change_cfg(**(lover or {})), cpu["geo"], tally)
    return w


def test_overtake_and_right_bias(cpu):
    geo = cpu["geo"]
    F, c = fdict(ppamd.default_follow_cfg()), ldict(ppamd.default_lane_change_cfg())
    tally = Tally()
    fr = overtake(geo)
    w = first_call(cpu, fr, tally=tally)
    # worked out: the follow update brakes the fast car behind the slow one (net gap 40 - 4.5) ...
    g = 40.0 - F["car_length"]
    v1 = FAST + sidm(F, FAST, FAST, SLOW, g) * 3 * DT
    assert np.abs(w["tr"]["speed"][0] - v1).max() <= TOL and (w["tr"]["speed"][1] == SLOW).all()
    # ... and on an empty neighbour lane it would be on a free road: nobody else gains or loses
    gain = sidm(F, v1, FAST) - sidm(F, v1, FAST, SLOW, g)
    assert np.abs(w["lc"]["gain"][0] - (gain - c["threshold"])).max() <= TOL and gain > 5
    # the slow car would only do its follower a favour: politeness times the same difference
    assert np.abs(w["lc"]["gain"][1] - (c["politeness"] * gain - c["threshold"])).max() <= TOL
    assert (w["lc"]["last_car"] == 1).all() and (w["lc"]["last_dir"] == -1).all()       # lane 0 under the tie rule
    assert (w["tr"]["lane"][0] == 0).all() and (w["tr"]["lane"][1] == 1).all()
    assert (w["lc"]["dir"][0] == -1).all() and (w["lc"]["n_changes"] == 1).all() and (w["lc"]["changes"][0] == 1).all()
    assert (w["lc"]["wait"][0] == c["min_interval_steps"]).all() and (w["lc"]["wait"][1] == 0).all()
    assert np.abs(w["tr"]["offset"][0] - 4.0).max() < 0.05 and (w["lc"]["home"][0] == 0).all()
    # right_bias > 0 lowers the threshold of lane + 1 and raises that of lane - 1: the change flips to lane 2
    # (the definitions' sign: the bias is ADDED to the threshold of a change to lane - 1); < 0 keeps lane 0
    w = first_call(cpu, fr, lover={"right_bias": 0.5}, tally=tally)
    assert (w["tr"]["lane"][0] == 2).all() and (w["lc"]["last_dir"] == 1).all()
    assert np.abs(w["lc"]["gain"][0] - (gain - c["threshold"] + 0.5)).max() <= TOL
    w = first_call(cpu, fr, lover={"right_bias": -0.5}, tally=tally)
    assert (w["tr"]["lane"][0] == 0).all() and (w["lc"]["last_dir"] == -1).all()
    # threshold +inf: nobody ever changes
    w = first_call(cpu, fr, lover={"threshold": INF}, tally=tally)
    assert not w["lc"]["last_car"].any() and np.isneginf(w["lc"]["gain"]).all() and not w["lc"]["dir"].any()
    same_bits({k: w["tr"][k] for k in ("lane", "seg", "t", "offset")},
              {k: fr["traffic"][k] for k in ("lane", "seg", "t", "offset")}, "threshold inf")
    tally.done("overtake", hand=True)


def test_unsafe_follower(cpu):
    """A 25 m/s car in each neighbour lane 6 m behind abreast (net gap 1.5 m < min_gap): the fast car
    may go nowhere; the slow car would make them brake harder than safe_brake; they cannot cut in."""
    geo = cpu["geo"]
    s1 = base_segment(geo, 1)[0]
    tally = Tally()
    fr = overtake(geo, extra=[(0, s1, 9.0, 0.0, 25.0), (2, s1, 9.0, 0.0, 25.0)])
    w = first_call(cpu, fr, tally=tally)
    assert not w["lc"]["last_car"].any() and not w["lc"]["n_changes"].any()
    assert np.isneginf(w["lc"]["gain"][0]).all() and (w["lc"]["dir"][0] == 0).all()
    assert np.isneginf(w["lc"]["gain"]).all()
    same_bits({k: w["tr"][k] for k in ("lane", "seg", "t", "offset")},
              {k: fr["traffic"][k] for k in ("lane", "seg", "t", "offset")}, "unsafe")
    tally.done("unsafe follower", hand=True)


def test_ego_as_follower(cpu):
    """The ego on lane 0, 15 m behind the fast car at 20 m/s: it would have to brake at max_brake, so
    lane 0 is refused and lane 2 chosen; cars that do not see the ego choose lane 0 again."""
    geo = cpu["geo"]
    F, c = fdict(ppamd.default_follow_cfg()), ldict(ppamd.default_lane_change_cfg())
    s1 = base_segment(geo, 1)[0]
    fr = overtake(geo, ego=(0, s1, 0.0, 0.0, 20.0))
    tally = Tally()
    w = first_call(cpu, fr, tally=tally)
    v1 = w["tr"]["speed"][0, 0]
    assert sidm(F, 20.0, c["ego_desired_speed"], v1, 15.0 - 4.5) < -c["safe_brake"]
    assert (w["tr"]["lane"][0] == 2).all() and (w["lc"]["last_car"] == 1).all() and (w["lc"]["last_dir"] == 1).all()
    w = first_call(cpu, fr, fover={"react_to_ego": 0}, tally=tally)
    assert (w["tr"]["lane"][0] == 0).all() and (w["lc"]["last_dir"] == -1).all()
    tally.done("ego as follower", hand=True)


def test_bounds(cpu):
    geo, NL = cpu["geo"], cpu["geo"].NL
    tally = Tally()
    # edge lanes
    w = first_call(cpu, overtake(geo, lane=0), tally=tally)
    assert (w["tr"]["lane"][0] == 1).all() and (w["lc"]["last_dir"] == 1).all()
    w = first_call(cpu, overtake(geo, lane=NL - 1), tally=tally)
    assert (w["tr"]["lane"][0] == NL - 2).all() and (w["lc"]["last_dir"] == -1).all()
    assert ((w["tr"]["lane"] >= 0) & (w["tr"]["lane"] < NL)).all()
    # a parked car (v0 = 0) 6.6 m behind the slow car never changes, whatever its follower would gain
    s1 = base_segment(geo, 1)[0]
    fr = frame_of(geo, 5, away(geo), [(1, s1, 15.0, 0.0, 0.0), (1, s1, 55.0, 0.0, SLOW)])
    w = first_call(cpu, fr, tally=tally)
    assert np.isneginf(w["lc"]["gain"][0]).all() and (w["lc"]["dir"][0] == 0).all() and (w["tr"]["lane"][0] == 1).all()
    # a car in transit never changes (min_interval_steps = 0: only the transit holds it), and a car
    # that is back on its home offset but still waits does not either
    for interval in (0, 250):
        w = frame_world(overtake(geo))
        lcfg = ppamd.default_lane_change_cfg(min_interval_steps=interval)
        calls = 0
        while True:
            follow_then_change(cpu["m"], w, 3, None, lcfg, geo, tally)
            calls += 1
            if calls == 1:
                assert (w["lc"]["last_car"] == 1).all()
                continue
            home = (w["tr"]["offset"][0] == w["lc"]["home"][0]).all()
            if not home or (interval and calls < 60):
                assert np.isneginf(w["lc"]["gain"][0]).all() and (w["lc"]["changes"][0] == 1).all(), calls
                assert home or not (w["lc"]["last_car"] == 1).any()
            if (home and not interval) or calls == 60:
                break
        assert 40 < calls <= 60
        if interval:
            assert (w["lc"]["wait"][0] == 250 - 59 * 3).all()
    tally.done("bounds", hand=True)


def tailgaters(geo, S, v0b):
    """Two cars 4.6 m (centre to centre) behind a slow car each, 300 m apart on lane 1: both brake at
    max_brake (the net gap is below gap_floor), so their gain is the free-road acceleration + 8."""
    s1 = base_segment(geo, 1)[0]
    rows = [(1, s1, 15.0, 0.0, 15.0), (1, s1, 19.6, 0.0, 3.0), (1, s1, 315.0, 0.0, v0b), (1, s1, 319.6, 0.0, 3.0)]
    return frame_of(geo, S, away(geo), rows)


def test_two_candidates_in_one_scene(cpu):
    geo = cpu["geo"]
    F, c = fdict(ppamd.default_follow_cfg()), ldict(ppamd.default_lane_change_cfg())
    tally = Tally()
    sur = lambda v0: sidm(F, v0 - F["max_brake"] * 3 * DT, v0) + F["max_brake"] - c["threshold"]
    # the same bits in both cars: the lower index changes
    w = first_call(cpu, tailgaters(geo, 5, 15.0), tally=tally)
    assert w["lc"]["gain"][0].tobytes() == w["lc"]["gain"][2].tobytes()
    assert np.abs(w["lc"]["gain"][0] - sur(15.0)).max() <= TOL
    assert (w["lc"]["last_car"] == 1).all() and (w["lc"]["n_changes"] == 1).all()
    assert (w["tr"]["lane"][0] == 0).all() and (w["tr"]["lane"][2] == 1).all()
    # a slower car is farther below its desired speed after the same braking: the larger surplus changes
    w = first_call(cpu, tailgaters(geo, 5, 12.0), tally=tally)
    assert sur(12.0) > sur(15.0) + 1e-3
    assert np.abs(w["lc"]["gain"][2] - sur(12.0)).max() <= TOL
    assert (w["lc"]["last_car"] == 3).all() and (w["lc"]["n_changes"] == 1).all()
    assert (w["tr"]["lane"][0] == 1).all() and (w["tr"]["lane"][2] == 0).all()
    assert (w["lc"]["changes"].sum(0) == 1).all()
    tally.done("two candidates", hand=True)


def test_no_traffic_touches_nothing(cpu):
    fr = frame_of(cpu["geo"], 4, away(cpu["geo"]), [])
    w = frame_world(fr)
    for a in w["lc"].values():
        a[...] = 7
    before = snap(w)
    ppamd.traffic_follow(cpu["m"], w["sc"], w["tr"], w["fo"])
    ppamd.traffic_lane_change(cpu["m"], w["sc"], w["tr"], w["fo"], w["lc"])
    same_bits(w["lc"], before["lc"], "no cars")
    same_bits({k: w["tr"][k] for k in TR_KEYS}, {k: before["tr"][k] for k in TR_KEYS}, "no cars")


def test_continuity_and_lateral_return(cpu):
    geo = cpu["geo"]
    c = ldict(ppamd.default_lane_change_cfg())
    w = frame_world(overtake(geo))
    tr = w["tr"]
    before = geo.car(tr["lane"][0], tr["seg"][0], tr["t"][0], tr["offset"][0])[0]
    tally = Tally()
    follow_then_change(cpu["m"], w, 3, geo=geo, tally=tally)
    assert (tr["lane"][0] == 0).all() and ((tr["t"][0] > 0) & (tr["t"][0] < 1)).all()
    after = geo.car(tr["lane"][0], tr["seg"][0], tr["t"][0], tr["offset"][0])[0]
    assert np.abs(after - before).max() <= 1e-9
    step = c["lateral_speed"] * 3 * DT
    need = np.ceil(np.abs(tr["offset"][0] - w["lc"]["home"][0]) / step).astype(int)
    assert (need == need[0]).all() and 40 < need[0] < 50
    for k in range(1, need[0] + 1):
        follow_then_change(cpu["m"], w, 3, geo=geo, tally=tally)
        at_home = tr["offset"][0] == w["lc"]["home"][0]
        assert at_home.all() if k == need[0] else not at_home.any(), k
    # a car that never changed lane keeps its offset bit for bit
    fr = overtake(geo, extra=[(2, base_segment(geo, 1)[0], 120.0, 0.2371, 12.0)])
    w = frame_world(fr)
    for _ in range(5):
        follow_then_change(cpu["m"], w, 3, geo=geo, tally=tally)
    assert w["tr"]["offset"][2].tobytes() == fr["traffic"]["offset"][2].tobytes() and (w["lc"]["changes"][2] == 0).all()
    tally.done("continuity", hand=True)


# ---- random frames -----------------------------------------------------------------------------------
def episode_start(m, S, n_cars, seed, **over):
    cfg = ppamd.default_episode_cfg(n_cars=n_cars, **over)
    sc, tr = ppamd.synth_episode_host(m, S, seed, 0, cfg)
    return sc, tr


@pytest.mark.parametrize("consume", [1, 3, 7])
def test_random_frames_vs_oracle(cpu, consume):
    """0 to 100 cars: world_lib.random_frame's frames (cars within 300 m, one in eight parked, the ego
    among them), the 100-car rollout starts and episode starts; three frames each, moved in between,
    so the later calls see cars in transit and waiting."""
    geo, m = cpu["geo"], cpu["m"]
    tally = Tally()
    lcfg = ppamd.default_lane_change_cfg(min_interval_steps=10)
    worlds = [frame_world(wl.random_frame(geo, 40, n, 3000 + 10 * n + consume)) for n in (0, 1, 2, 5, 12, 33)]
    worlds.append(frame_world(wl.random_frame(geo, 12, 100, 3100 + consume)))
    worlds.append(world(*many_car_traffic(m, 12, 31 + consume)))
    worlds.append(world(*many_car_traffic(m, 12, 41 + consume, dense=True)))
    worlds.append(world(*episode_start(m, 64, 12, 500 + consume)))
    worlds.append(world(*episode_start(m, 64, 30, 600 + consume, extra_gap=5.0)))
    begun = 0
    for w in worlds:
        for _ in range(3):
            follow_then_change(m, w, consume, None, lcfg, geo, tally)
            begun += int((w["lc"]["last_car"] > 0).sum())
            move(geo, w["tr"], consume)
    print(f"consume {consume}: {begun} changes begun")
    assert begun >= 20
    tally.done(f"random frames, consume {consume}")


def test_untouched_scenes_and_reused_state(cpu):
    geo, m = cpu["geo"], cpu["m"]
    fr = wl.random_frame(geo, 16, 12, 91)
    w = frame_world(fr)
    ppamd.traffic_follow(m, w["sc"], w["tr"], w["fo"])
    w["fo"]["started"][::2] = 0                          # half of the scenes: not started by follow
    for a in w["lc"].values():
        a[..., ::2] = 5
    before = snap(w)
    ppamd.traffic_lane_change(m, w["sc"], w["tr"], w["fo"], w["lc"])
    for k in TR_KEYS:
        assert w["tr"][k][:, ::2].tobytes() == before["tr"][k][:, ::2].tobytes(), k
    for k, a in w["lc"].items():
        assert a[..., ::2].tobytes() == before["lc"][k][..., ::2].tobytes(), k
    assert (w["lc"]["started"][1::2] == 1).all()
    want_tr, want_lc, amb = oracle_call(geo, ppamd.default_follow_cfg(), ppamd.default_lane_change_cfg(), before["sc"],
                                        before["tr"], before["fo"], before["lc"], 3)
    t = Tally()
    t.check(w["tr"], w["lc"], want_tr, want_lc, amb, 12)
    # a used state with `started` zeroed behaves as a fresh one
    used = frame_world(wl.random_frame(geo, 16, 12, 92))
    for _ in range(4):
        follow_then_change(m, used, 3)
        move(geo, used["tr"], 3)
    assert used["lc"]["n_changes"].any()
    a, b = frame_world(fr), frame_world(fr)
    a["lc"] = used["lc"]
    a["lc"]["started"][:] = 0
    for _ in range(4):
        for x in (a, b):
            follow_then_change(m, x, 3)
            move(geo, x["tr"], 3)
    same_bits({k: a["tr"][k] for k in TR_KEYS}, {k: b["tr"][k] for k in TR_KEYS}, "reused traffic")
    same_bits({k: v for k, v in a["lc"].items() if k not in ("arc", "gain", "dir")},
              {k: v for k, v in b["lc"].items() if k not in ("arc", "gain", "dir")}, "reused state")
    same_bits(a["lc"], b["lc"], "reused state, records")


# ---- the closed loop ----------------------------------------------------------------------------------
# the episode cfg of the closed-loop test: the default start suffices (changes begin in 255 of the 256
# scenes within the 200 frames), so no field is overridden
LOOP_CFG = {}


def lane_neighbours(geo, F, sc, tr, j_s):
    """For the (car, scene) pairs j_s after a change: net gaps to the nearest vehicle ahead and behind
    on the car's lane (the ego where it occupies it) and the follower's (speed, v0 or None for the
    ego), from positions alone."""
    out = []
    J = int(tr["n_cars"])
    arc = geo.cum0[tr["lane"][:J], tr["seg"][:J]] + tr["t"][:J] * geo.L[tr["lane"][:J], tr["seg"][:J]]
    arc_e, dist_e = wl.FollowOracle(geo, ppamd.default_follow_cfg()).ego_on_lanes(np.stack([sc["ego_x"], sc["ego_y"]], -1))
    for j, s in j_s:
        l = tr["lane"][j, s]
        loop = geo.tot[l]
        ahead, behind, foll = INF, INF, None
        for m in range(J + 1):
            if m == j or (m < J and tr["lane"][m, s] != l) or (m == J and not dist_e[l, s] <= F["lateral_reach"]):
                continue
            am, ln = (arc[m, s], F["car_length"]) if m < J else (arc_e[l, s], F["ego_length"])
            ca, cb = (am - arc[j, s]) % loop, (arc[j, s] - am) % loop
            ahead = min(ahead, ca - (F["car_length"] + ln) / 2)
            if cb - (F["car_length"] + ln) / 2 < behind:
                behind, foll = cb - (F["car_length"] + ln) / 2, m
        out.append((ahead, behind, foll))
    return out


def test_closed_loop(cpu):
    """The C restatement of the planner one frame at a time with the host twins of follow, lane change
    and judge (test_episode's drive), 256 scenes x 200 frames: every change that begins leaves net
    gaps >= min_gap on its new lane and a new follower that brakes no harder than safe_brake; lanes
    stay in range, waits are honoured, no car in transit begins a change."""
    geo, m = cpu["geo"], cpu["m"]
    S, frames, consume = 256, 200, 3
    fcfg, lcfg = ppamd.default_follow_cfg(), ppamd.default_lane_change_cfg()
    F, c = fdict(fcfg), ldict(lcfg)
    ecfg = ppamd.default_episode_cfg(**LOOP_CFG)
    n = ecfg.n_cars
    judge, follow = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n)
    sc, tr = ppamd.synth_episode_host(m, S, 7, 0, ecfg, judge=judge, follow=follow)
    lc = ppamd.alloc_lane_change(S, n)
    olib = oracle_lib.load_oracle()
    prm = ppamd.default_params(n_speeds=1)
    changes = 0
    worst_gap, worst_brake = INF, INF
    for f in range(frames):
        ppamd.traffic_follow(m, sc, tr, follow, consume=consume, cfg=fcfg)
        before_wait, before_off = lc["wait"].copy(), tr["offset"].copy()
        started = lc["started"].copy()
        ppamd.traffic_lane_change(m, sc, tr, follow, lc, consume=consume, fcfg=fcfg, cfg=lcfg)
        assert ((tr["lane"] >= 0) & (tr["lane"] < geo.NL)).all()
        ss = np.nonzero(lc["last_car"])[0]
        j_s = [(int(lc["last_car"][s]) - 1, int(s)) for s in ss]
        for (j, s), (ahead, behind, foll) in zip(j_s, lane_neighbours(geo, F, sc, tr, j_s)):
            changes += 1
            assert before_wait[j, s] - consume <= 0 or not started[s], (f, j, s)
            # it was on its home offset before this call (so after this call's lateral move too)
            assert before_off[j, s] == lc["home"][j, s], (f, j, s)
            assert lc["wait"][j, s] == c["min_interval_steps"]
            if ahead <= F["horizon"]:
                assert ahead >= F["min_gap"] - 1e-9, (f, j, s, ahead)
                worst_gap = min(worst_gap, ahead)
            if foll is not None and behind <= F["horizon"]:
                assert behind >= F["min_gap"] - 1e-9, (f, j, s, behind)
                worst_gap = min(worst_gap, behind)
                vj = tr["speed"][j, s]
                if foll == n:
                    a = sidm(F, sc["ego_speed_mph"][s] / MPH, c["ego_desired_speed"], vj, behind)
                elif follow["desired"][foll, s] > 0:
                    a = sidm(F, tr["speed"][foll, s], follow["desired"][foll, s], vj, behind)
                else:
                    a = 0.0
                assert a >= -c["safe_brake"] - 1e-9, (f, j, s, a)
                worst_brake = min(worst_brake, a)
        pre_sc, pre_tr = oracle_lib.copy_state(sc, tr)
        lg = oracle_lib.oracle_rollout(olib, cpu["wx"], cpu["wy"], sc, tr, prm, 1, consume, 400.0)
        res = {"n_out": np.ascontiguousarray(lg["n_out"][0]), "next_x": np.ascontiguousarray(lg["plan_x"][0]),
               "next_y": np.ascontiguousarray(lg["plan_y"][0])}
        ppamd.judge_frame(m, pre_sc, pre_tr, res, judge, consume=consume)
    scenes = int((lc["n_changes"] > 0).sum())
    assert changes == int(lc["n_changes"].sum()) == int(lc["changes"].sum())
    j = ppamd.judge_to_numpy(judge)
    print(f"closed loop {LOOP_CFG}: {changes} changes in {scenes} of {S} scenes over {frames} frames; smallest new "
          f"net gap {worst_gap:.2f} m, hardest new-follower braking {worst_brake:.2f} m/s^2; "
          f"{int(((j['flags'] & ppamd.INC_COLLISION) != 0).sum())} scenes collide")
    assert scenes >= 10


def test_passing(cpu):
    """The overtake pair alone for 600 frames of follow + lane change + move: with lane changes the
    fast car ends more than a car length ahead of the slow one; with threshold +inf it never is."""
    geo, m = cpu["geo"], cpu["m"]
    fcfg = ppamd.default_follow_cfg(react_to_ego=0)
    o = wl.FollowOracle(geo, fcfg)

    def lead_of_fast(tr):                                # arcs of both cars on lane 1's polyline
        p = geo.car(tr["lane"][:2], tr["seg"][:2], tr["t"][:2], tr["offset"][:2])[0]
        a = np.stack([o.ego_on_lanes(p[k])[0][1] for k in (0, 1)])
        d = a[0] - a[1]
        return (d + geo.tot[1] / 2) % geo.tot[1] - geo.tot[1] / 2

    ends = {}
    for name, thr in (("on", 0.2), ("off", INF)):
        w = frame_world(overtake(geo, S=3))
        lcfg = ppamd.default_lane_change_cfg(threshold=thr)
        ahead = []
        for _ in range(600):
            follow_then_change(m, w, 3, fcfg, lcfg)
            move(geo, w["tr"], 3)
            ahead.append(lead_of_fast(w["tr"]))
        ends[name] = np.array(ahead)
    print(f"passing: fast car ahead by {ends['on'][-1][0]:.1f} m with lane changes, at most {ends['off'].max():.1f} m without")
    assert (ends["on"][-1] > 4.5).all()
    assert (ends["off"] < 0).all()


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors(cpu):
    geo = cpu["geo"]
    fr = overtake(geo, S=2)
    sc = ppamd.add_car_table(wl.scenes_of(fr))
    tr = fr["traffic"]
    b, T = ppamd.scene_struct(sc), ppamd.traffic_struct(tr)
    follow, lc = ppamd.alloc_follow(2, 2), ppamd.alloc_lane_change(2, 2)
    ppamd.traffic_follow(cpu["m"], sc, tr, follow)
    Fs, Ls = ppamd.follow_struct(follow), ppamd.lane_change_struct(lc)
    prm = ppamd.default_params(n_speeds=1)
    res = ppamd.alloc_result(2, prm)
    R = ppamd.result_struct(res)
    rc = ppamd.RolloutCfg(1, 3, 100.0)
    before = {k: tr[k].copy() for k in TR_KEYS}
    fok, ok = ppamd.default_follow_cfg(), ppamd.default_lane_change_cfg()
    ref = lambda x: C.byref(x) if x is not None else None

    def call(cfg=ok, fcfg=fok, consume=3, state=Ls, fstate=Fs, host=True, scenes=b, traffic=T, handle=cpu["m"].handle):
        if host:
            return ppamd.lib.pp_traffic_lane_change_host(handle, ref(scenes), ref(traffic), consume, ref(fcfg),
                                                         ref(fstate), ref(cfg), ref(state))
        return ppamd.lib.pp_traffic_lane_change(handle, ref(scenes), ref(traffic), consume, ref(fcfg), ref(fstate),
                                                ref(cfg), ref(state), 0, None)

    def rollout(cfg=ok, state=Ls, fcfg=fok, fstate=Fs):
        return ppamd.lib.pp_rollout_lane_changing(cpu["m"].handle, C.byref(b), C.byref(T), C.byref(prm), C.byref(rc),
                                                  C.byref(R), None, 0, None, None, None, ref(fcfg), ref(fstate),
                                                  ref(cfg), ref(state))

    assert [getattr(ok, k) for k, _ in ppamd.LaneChangeCfg._fields_[:-1]] == [0.3, 0.2, 0.0, 3.0, 1.5, 22.2, 250]
    nan = float("nan")
    bad = [{"politeness": -0.1}, {"politeness": nan}, {"threshold": nan}, {"right_bias": nan}, {"safe_brake": 0.0},
           {"safe_brake": -1.0}, {"safe_brake": nan}, {"lateral_speed": 0.0}, {"lateral_speed": -1.0},
           {"lateral_speed": nan}, {"ego_desired_speed": 0.0}, {"ego_desired_speed": -2.0}, {"ego_desired_speed": nan},
           {"min_interval_steps": -1}]
    fbad = [{"max_acc": 0.0}, {"max_brake": -8.0}, {"gap_floor": 0.0}, {"horizon": nan}, {"car_length": -0.1}]
    for host in (True, False):       # every check comes before any HIP call
        for over in bad:
            assert call(ppamd.default_lane_change_cfg(**over), host=host) == -1, over
        for over in fbad:
            assert call(fcfg=ppamd.default_follow_cfg(**over), host=host) == -1, over
        for kw in ({"cfg": None}, {"fcfg": None}, {"state": None}, {"fstate": None}, {"scenes": None},
                   {"traffic": None}, {"handle": None}, {"consume": 0}, {"consume": -3}):
            assert call(host=host, **kw) == -1, kw
        for hole in [k for k, _, _ in ppamd.LANE_CHANGE_FIELDS]:
            holed = ppamd.lane_change_struct(lc)
            setattr(holed, hole, None)
            assert call(state=holed, host=host) == -1, hole
        for hole in [k for k, _, _ in ppamd.FOLLOW_FIELDS]:
            holed = ppamd.follow_struct(follow)
            setattr(holed, hole, None)
            assert call(fstate=holed, host=host) == -1, hole
        nospeed = ppamd.scene_struct(sc)
        nospeed.ego_speed_mph = None
        assert call(scenes=nospeed, host=host) == -1
        notr = ppamd.traffic_struct(tr)
        notr.offset = None
        assert call(traffic=notr, host=host) == -1
    for over in bad:
        assert rollout(ppamd.default_lane_change_cfg(**over)) == -1, over
    assert rollout(cfg=None) == -1 and rollout(state=None) == -1            # one without the other
    assert rollout(fcfg=None) == -1 and rollout(fstate=None) == -1
    holed = ppamd.lane_change_struct(lc)
    holed.arc = None
    assert rollout(state=holed) == -1
    assert not any(a.any() for a in lc.values())
    for k in TR_KEYS:
        assert tr[k].tobytes() == before[k].tobytes()
    wide = ppamd.default_lane_change_cfg(politeness=0.0, threshold=INF, right_bias=-3.0, min_interval_steps=0)
    assert call(wide) == 0                                                  # the edges of the allowed ranges


# ---- the four-lane build ------------------------------------------------------------------------------
def test_four_lane_build_host():
    """In the 4-lane library a car on lane 2 changes to lane 3 (tests/lane_change_lanes4_cases.py, a
    child process: a process loads one PP_NUM_LANES)."""
    run_lanes4("lane_change_lanes4_cases.py", "not gpu")


# ---- GPU ------------------------------------------------------------------------------------------------
def world_bits(a, b, what):
    for part in ("tr", "fo", "lc"):
        same_bits({k: v for k, v in a[part].items() if k != "n_cars"},
                  {k: v for k, v in b[part].items() if k != "n_cars"}, f"{what} {part}")


def device_equals_host(m, geo, sc, tr, dev, what, consume=3, rounds=3, lcfg=None):
    """`rounds` frames of follow + lane change + move, device against host twin: every traffic and
    state array bit for bit after every call. Returns the changes begun."""
    import torch
    lcfg = lcfg if lcfg is not None else ppamd.default_lane_change_cfg(min_interval_steps=10)
    h, d = world(sc, tr), world(sc, tr, dev)
    begun = 0
    for r in range(rounds):
        follow_then_change(m, h, consume, None, lcfg)
        follow_then_change(m, d, consume, None, lcfg)
        torch.cuda.synchronize()
        got = snap(d)
        world_bits(got, h, f"{what} round {r}")
        begun += int((h["lc"]["last_car"] > 0).sum())
        move(geo, h["tr"], consume)
        for k in ("seg", "t"):
            d["tr"][k] = up(h["tr"][k], dev)
    return begun


@pytest.mark.gpu
class TestLaneChangeGPU:
    @pytest.fixture(scope="class")
    def env(self, cpu):
        import torch
        return dict(cpu, torch=torch, dev=torch.device("cuda", 0))

    @pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
    def test_device_equals_host_twin_bit_for_bit(self, env, S):
        """0, 1, 2, 12, 33 and 100 cars (the short last block of cars included), the hand-made overtake
        frame and an episode start, at the wave and block edges of S."""
        geo, m, dev = env["geo"], env["m"], env["dev"]
        begun = 0
        for n_cars, consume in ((0, 3), (1, 1), (2, 3), (12, 3), (33, 7), (100, 3)):
            fr = wl.random_frame(geo, S, n_cars, 7000 + n_cars + S)
            begun += device_equals_host(m, geo, wl.scenes_of(fr), fr["traffic"], dev, f"random {n_cars}", consume)
        fr = overtake(geo, S=S)
        begun += device_equals_host(m, geo, wl.scenes_of(fr), fr["traffic"], dev, "overtake")
        sc, tr = episode_start(m, S, 30, 800 + S, extra_gap=5.0)
        begun += device_equals_host(m, geo, sc, tr, dev, "episode")
        assert begun >= S

    def rollout_state(self, env, S, F, seed=11, n=12):
        t, dev = env["torch"], env["dev"]
        prm = ppamd.default_params(n_speeds=1)
        judge, follow = ppamd.alloc_judge(S, xp="torch", device=dev), ppamd.alloc_follow(S, n, xp="torch", device=dev)
        ppamd.plan_reset(env["m"])
        d, g = ppamd.synth_episode(env["m"], S, seed=seed, cfg=ppamd.default_episode_cfg(n_cars=n, extra_gap=5.0),
                                   device=0, judge=judge, follow=follow)
        t.cuda.synchronize()
        return {"d": d, "g": g, "prm": prm, "res": ppamd.alloc_result(S, prm, xp="torch", device=dev),
                "lg": ppamd.alloc_log(F, S, 50, xp="torch", device=dev), "judge": judge, "follow": follow,
                "lc": ppamd.alloc_lane_change(S, n, xp="torch", device=dev)}

    def collect(self, env, r):
        env["torch"].cuda.synchronize()
        return [to_np(x) for x in (r["d"], {k: v for k, v in r["g"].items() if k != "n_cars"}, r["res"], r["lg"],
                                   r["follow"], r["lc"])] + [ppamd.judge_to_numpy(r["judge"])]

    def same_runs(self, a, b, names=("scenes", "traffic", "result", "log", "follow", "lane change", "judge")):
        for what, x, y in zip(("scenes", "traffic", "result", "log", "follow", "lane change", "judge"), a, b):
            if what in names:
                same_bits({k: v for k, v in x.items() if v is not None}, {k: v for k, v in y.items() if v is not None}, what)

    def test_one_call_equals_one_frame_calls(self, env):
        """One 40-frame pp_rollout_lane_changing call equals 40 one-frame calls, bit for bit (S = 384)."""
        S, F = 384, 40
        runs = []
        for calls in (1, F):
            r = self.rollout_state(env, S, F, n=24)
            for c in range(calls):
                part = r["lg"] if calls == 1 else {k: v[c:c + 1] for k, v in r["lg"].items()}
                ppamd.rollout_lane_changing(env["m"], r["d"], r["g"], r["prm"], r["res"], r["follow"], r["lc"],
                                            F // calls, 3, 100.0, part, judge=r["judge"])
            runs.append(self.collect(env, r))
        self.same_runs(*runs)
        assert runs[0][5]["n_changes"].sum() >= 10 and (runs[0][5]["started"] == 1).all()

    def test_disabled_equals_rollout_reactive(self, env):
        """threshold = +inf, and NULL lcfg / lstate: telemetry, car table, traffic, result, log, judge and
        follow state equal pp_rollout_reactive's bit for bit over 40 frames at S = 1000."""
        S, F = 1000, 40
        runs = []
        for mode in ("reactive", "inf", "null"):
            r = self.rollout_state(env, S, F, n=24)
            if mode == "reactive":
                ppamd.rollout_reactive(env["m"], r["d"], r["g"], r["prm"], r["res"], r["follow"], F, 3, 100.0, r["lg"],
                                       judge=r["judge"])
            else:
                ppamd.rollout_lane_changing(env["m"], r["d"], r["g"], r["prm"], r["res"], r["follow"],
                                            r["lc"] if mode == "inf" else None, F, 3, 100.0, r["lg"], judge=r["judge"],
                                            lcfg=ppamd.default_lane_change_cfg(threshold=INF))
            runs.append(self.collect(env, r))
        keep = ("scenes", "traffic", "result", "log", "follow", "judge")
        self.same_runs(runs[0], runs[1], keep)
        self.same_runs(runs[0], runs[2], keep)
        assert (runs[1][5]["started"] == 1).all() and not runs[1][5]["n_changes"].any()
        assert not any(a.any() for a in runs[2][5].values())

    def test_dense_traffic_device_equals_host_frame_by_frame(self, env):
        """Dense 100-car traffic, 64 scenes x 150 frames of pp_rollout_lane_changing (judge on), one frame
        per call; the host twins recompute follow, lane change and judge from the GPU's own pre-frame
        state: every field of the three states and the traffic bit for bit."""
        t, dev = env["torch"], env["dev"]
        S, F, n = 64, 150, 100
        sc, tr = many_car_traffic(env["m"], S, 23, dense=True)
        prm = ppamd.default_params(n_speeds=1)
        jcfg, fcfg = ppamd.default_judge_cfg(), ppamd.default_follow_cfg()
        lcfg = ppamd.default_lane_change_cfg(min_interval_steps=30)
        ppamd.plan_reset(env["m"])
        d = {k: up(v, dev) for k, v in sc.items()}
        g = {k: up(v, dev) for k, v in tr.items()}
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        follow = ppamd.alloc_follow(S, n, xp="torch", device=dev)
        lc = ppamd.alloc_lane_change(S, n, xp="torch", device=dev)
        hj, hf, hl = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n), ppamd.alloc_lane_change(S, n)
        for f in range(F):
            pre_sc, pre_tr = to_np(d), to_np(g)
            ppamd.rollout_lane_changing(env["m"], d, g, prm, res, follow, lc, 1, 3, 400.0, judge=judge, jcfg=jcfg,
                                        fcfg=fcfg, lcfg=lcfg)
            t.cuda.synchronize()
            ppamd.traffic_follow(env["m"], pre_sc, pre_tr, hf, consume=3, cfg=fcfg)
            ppamd.traffic_lane_change(env["m"], pre_sc, pre_tr, hf, hl, consume=3, fcfg=fcfg, cfg=lcfg)
            same_bits(ppamd.follow_to_numpy(follow), hf, f"frame {f} follow")
            same_bits(ppamd.lane_change_to_numpy(lc), hl, f"frame {f} lane change")
            got = to_np(g)
            for k in ("lane", "offset", "speed"):        # seg and t: k_sim has moved the cars since
                assert got[k].tobytes() == pre_tr[k].tobytes(), f"frame {f} {k}"
            plan = {k: res[k].cpu().numpy() for k in ("n_out", "next_x", "next_y")}
            ppamd.judge_frame(env["m"], pre_sc, pre_tr, plan, hj, consume=3, cfg=jcfg)
        same_bits(ppamd.judge_to_numpy(judge), ppamd.judge_to_numpy(hj), "dense judge")
        print(f"dense 100 cars, {S} scenes x {F} frames: {int(hl['n_changes'].sum())} changes begun")
        assert hl["n_changes"].sum() >= S

    def test_four_lane_build_device(self):
        run_lanes4("lane_change_lanes4_cases.py", "gpu")
