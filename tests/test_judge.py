"""The rollout judge (include/pp.h pp_judge_frame, pp_rollout_judged; csrc/pp_judge.h): incidents
of a closed-loop drive — collision, speed, acceleration, jerk, off-lane.

The definitions are the project's own (DESIGN.md "Rollout judge"), modelled on the published rules
of the simulator the reference planner was written for; the simulator is not available, so nothing
here is compared with it. The oracle is the NumPy restatement of those definitions below, written
independently of the library's code: it keeps the whole velocity history (no ring), finds a car by
arc length along its lane (no segment walk), tests rectangles by projecting their corners on the
four axes, and scans every segment of every lane polyline for the off-lane distance (no hint).

Tolerances. Continuous outputs within TOL = 1e-8 absolute: coordinates up to ~3e3 m carry at most
5e-13 m of rounding, /dt makes that 2.5e-11 m/s, the four-term jerk stencil divided by
Wa Wj dt^2 (= 0.2 for the defaults) at most 5e-10; the margin over that is x20. Flags, counts and
first steps are exact, except that a step whose ORACLE value lies within TIE = 1e-6 of its
threshold (sep vs 0, speed, acc and jerk vs their limits, dl vs lane_tol) is excluded from the
exact comparison: the library may decide it either way. The excluded share is asserted to be at
most 1 % of the judged steps in every test, and zero in the hand-made cases.

An episode's v_0 is 0 (include/pp.h), so a drive that starts at speed registers an ACC incident at
step acc_window; the hand-made clean drives start from rest."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import DT, TOL, Geo, base_segment, many_car_traffic, run_lanes4, same_bits, up

TIE = 1e-6
KINDS = len(ppamd.INC_KINDS)
COL, SPD, ACC, JRK, OFF = range(KINDS)

def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in ppamd.JudgeCfg._fields_}


def perp(a):
    return np.stack([a[..., 1], -a[..., 0]], -1)


def corners(c, ax, hl, hw):
    ay = perp(ax)
    return np.stack([c + sl * hl * ax + sw * hw * ay for sl in (-1, 1) for sw in (-1, 1)], -2)


def rect_sep(pe, he, ehl, ehw, pc, uc, chl, chw):
    """Separating-axis separation of ego (centre pe [S, 2], axis he) and cars (pc, uc [J, S, 2]) by
    projecting the eight corners on the four axes: the largest gap between the two intervals."""
    ce = np.broadcast_to(corners(pe, he, ehl, ehw), pc.shape[:-1] + (4, 2))
    cc = corners(pc, uc, chl, chw)
    sep = None
    for a in (np.broadcast_to(he, pc.shape), np.broadcast_to(perp(he), pc.shape), uc, perp(uc)):
        e = (ce * a[..., None, :]).sum(-1)
        c = (cc * a[..., None, :]).sum(-1)
        gap = np.maximum(c.min(-1) - e.max(-1), e.min(-1) - c.max(-1))
        sep = gap if sep is None else np.maximum(sep, gap)
    return sep


class Oracle:
    """The issue's definitions over S scenes at once; every scene at the same step number."""

    def __init__(self, geo, S, cfg):
        self.g, self.S, self.c = geo, S, cfg_dict(cfg)
        self.n = 0
        self.V = [np.zeros((S, 2))]                    # v_0 = 0; the whole history
        self.head = None
        z = lambda dt=float: np.zeros(S, dt)
        self.dist, self.clean, self.max_mph, self.max_acc, self.max_jerk = z(), z(), z(), z(), z()
        self.min_sep = np.full(S, np.inf)
        self.cnt, self.namb, self.first = (np.zeros((KINDS, S), int) for _ in range(3))
        self.first_amb = np.zeros((KINDS, S), bool)    # a near-tie step came before the first sure one
        self.first_car, self.first_car_ok = z(int), np.ones(S, bool)
        self.run_lo, self.run_hi = z(int), z(int)
        self.violated, self.clean_ok = z(bool), np.ones(S, bool)
        self.excluded = self.judged = 0

    def frame(self, x0, y0, yaw_deg, px, py, n_out, tr, consume):
        g, c, S = self.g, self.c, self.S
        Wa, Wj = c["acc_window"], c["jerk_window"]
        if self.n == 0:
            a = np.asarray(yaw_deg) * np.pi / 180
            self.head = np.stack([np.cos(a), np.sin(a)], -1)
        kk = np.minimum(n_out, consume)
        pp = np.stack([x0, y0], -1).astype(float)
        J = tr["n_cars"]
        for i in range(1, consume + 1):
            idx = np.maximum(np.minimum(i, kk) - 1, 0)
            p = np.where((kk > 0)[:, None], np.stack([px[idx, np.arange(S)], py[idx, np.arange(S)]], -1),
                         np.stack([x0, y0], -1))
            d = p - pp
            ln = np.sqrt((d ** 2).sum(-1))
            v = d / DT
            self.V.append(v)
            self.n += 1
            n = self.n
            self.dist = self.dist + ln
            mv = ln > 0
            self.head = np.where(mv[:, None], d / np.where(mv, ln, 1.0)[:, None], self.head)
            sure, amb = np.zeros((KINDS, S), bool), np.zeros((KINDS, S), bool)

            def limit(k, val, thr):
                sure[k] = val > thr + TIE
                amb[k] = np.abs(val - thr) <= TIE

            mph = np.sqrt((v ** 2).sum(-1)) * 2.237
            self.max_mph = np.maximum(self.max_mph, mph)
            limit(SPD, mph, c["speed_limit_mph"])
            if n >= Wa:
                acc = (self.V[n] - self.V[n - Wa]) / (Wa * DT)
                am = np.sqrt((acc ** 2).sum(-1))
                self.max_acc = np.maximum(self.max_acc, am)
                limit(ACC, am, c["max_acc"])
                if n >= Wa + Wj:
                    acc2 = (self.V[n - Wj] - self.V[n - Wj - Wa]) / (Wa * DT)
                    jm = np.sqrt((((acc - acc2) / (Wj * DT)) ** 2).sum(-1))
                    self.max_jerk = np.maximum(self.max_jerk, jm)
                    limit(JRK, jm, c["max_jerk"])
            if J > 0:
                lane, off, sp = tr["lane"][:J], tr["offset"][:J], tr["speed"][:J]
                seg, t = g.place(lane, tr["seg"][:J], tr["t"][:J], sp * DT * i)
                pc, uc = g.car(lane, seg, t, off)
                sep = rect_sep(p, self.head, c["ego_length"] / 2, c["ego_width"] / 2, pc, uc,
                               c["car_length"] / 2, c["car_width"] / 2)
                self.min_sep = np.minimum(self.min_sep, sep.min(axis=0))
                sure[COL] = (sep < -TIE).any(axis=0)
                amb[COL] = ~sure[COL] & (sep <= TIE).any(axis=0)
                newc = sure[COL] & (self.first[COL] == 0)
                self.first_car = np.where(newc, np.argmax(sep <= 0, axis=0) + 1, self.first_car)
                self.first_car_ok &= ~(newc & ((np.abs(sep) <= TIE).any(axis=0) | self.first_amb[COL]))
            dl = g.lane_dist(p)
            o_sure, o_amb = dl > c["lane_tol"] + TIE, np.abs(dl - c["lane_tol"]) <= TIE
            self.run_lo = np.where(o_sure, self.run_lo + 1, 0)
            self.run_hi = np.where(o_sure | o_amb, self.run_hi + 1, 0)
            sure[OFF] = self.run_lo > c["off_lane_steps"]
            amb[OFF] = (self.run_hi > c["off_lane_steps"]) & ~sure[OFF]
            for k in range(KINDS):
                self.first_amb[k] |= amb[k] & (self.first[k] == 0)
                self.first[k] = np.where(sure[k] & (self.first[k] == 0), n, self.first[k])
                self.cnt[k] += sure[k]
                self.namb[k] += amb[k]
            amb_any = amb.any(axis=0) | o_amb
            self.clean_ok &= ~(amb_any & ~self.violated)
            self.violated |= sure.any(axis=0)
            self.clean = np.where(self.violated, self.clean, self.dist)
            self.excluded += int(amb_any.sum())
            self.judged += S
            pp = p


def close(got, want, what):
    same = (got == want)                               # equal infinities (min_sep with no cars)
    err = np.abs(np.where(same, 0.0, got - np.where(same, 0.0, want)))
    assert np.all(err <= TOL), (what, float(np.nanmax(err)), np.argmax(err))
    return float(err.max(initial=0.0))


def compare(got, o, hand=False):
    """The library's judge state against the oracle's, under the module docstring's rules."""
    assert (got["steps"] == o.n).all()
    sure_f, may_f = np.zeros(o.S, np.uint32), np.zeros(o.S, np.uint32)
    for k in range(KINDS):
        lo, hi = o.cnt[k], o.cnt[k] + o.namb[k]
        assert ((got["count"][k] >= lo) & (got["count"][k] <= hi)).all(), (ppamd.INC_KINDS[k], got["count"][k], lo, hi)
        ex = ~o.first_amb[k]
        np.testing.assert_array_equal(got["first_step"][k][ex], o.first[k][ex], err_msg=ppamd.INC_KINDS[k])
        sure_f |= (lo > 0).astype(np.uint32) << k
        may_f |= (hi > 0).astype(np.uint32) << k
    assert not (got["flags"] & ~may_f).any() and not (sure_f & ~got["flags"]).any(), (got["flags"], sure_f, may_f)
    np.testing.assert_array_equal(got["first_car"][o.first_car_ok], o.first_car[o.first_car_ok])
    ex = o.run_lo == o.run_hi
    np.testing.assert_array_equal(got["off_run"][ex], o.run_lo[ex])
    worst = 0.0
    for k, w in (("dist", o.dist), ("min_sep", o.min_sep), ("max_speed_mph", o.max_mph), ("max_acc", o.max_acc),
                 ("max_jerk", o.max_jerk), ("head_x", o.head[:, 0]), ("head_y", o.head[:, 1])):
        worst = max(worst, close(got[k], w, k))
    worst = max(worst, close(got["clean_dist"][o.clean_ok], o.clean[o.clean_ok], "clean_dist"))
    for n in range(max(0, o.n - ppamd.JUDGE_RING + 1), o.n + 1):       # the ring holds the last 64 velocities
        k = n % ppamd.JUDGE_RING
        worst = max(worst, close(got["ring_vx"][k], o.V[n][:, 0], f"ring_vx {n}"),
                    close(got["ring_vy"][k], o.V[n][:, 1], f"ring_vy {n}"))
    share = o.excluded / max(o.judged, 1)
    print(f"judge vs oracle: {o.n} steps x {o.S} scenes, max |d| {worst:.2e}, near-tie steps {o.excluded} "
          f"({100 * share:.3f} %)")
    assert share <= 0.01, share
    if hand:
        assert o.excluded == 0
    return worst


# ---- inputs -------------------------------------------------------------------------------------
def track(geo, S, speeds, lane=1, lat=0.0):
    """Straight drive along the base segment of `lane`, `lat` metres to its right: points [n + 1, S, 2]
    (P[0] the start) with step speeds `speeds`; scene s starts 0.013 (s % 97) m farther on."""
    _, o, u, nrm = base_segment(geo, lane)
    s_along = np.concatenate([[0.0], np.cumsum(np.asarray(speeds, float) * DT)])
    shift = 0.013 * (np.arange(S) % 97)
    P = o[None, None] + (s_along[:, None] + shift[None])[..., None] * u + lat * nrm
    yaw = np.full(S, np.degrees(np.arctan2(u[1], u[0])))
    return P, yaw


def cars_on(geo, S, rows):
    """Traffic from rows (lane, seg, metres from the segment's start, offset, speed), same in every scene."""
    tr = ppamd.alloc_traffic(S, n=max(len(rows), 1))
    for j, (lane, seg, s_along, off, v) in enumerate(rows):
        sg, t = geo.place(np.array([lane]), np.array([seg]), np.array([0.0]), np.array([float(s_along)]))
        tr["lane"][j], tr["seg"][j], tr["t"][j], tr["offset"][j], tr["speed"][j] = lane, sg[0], t[0], off, v
    tr["n_cars"] = len(rows)
    return tr


def frames_of(geo, P, yaw, tr, consume, n_out=None):
    """Frames of `consume` steps over the track P; the traffic moves between them (same inputs for the
    library and the oracle; `place` is only how these inputs are made)."""
    steps = P.shape[0] - 1
    assert steps % consume == 0
    J = tr["n_cars"]
    out = []
    for f in range(steps // consume):
        t = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in tr.items()}
        if J and f:
            sg, tt = geo.place(tr["lane"][:J], tr["seg"][:J], tr["t"][:J], tr["speed"][:J] * DT * consume * f)
            t["seg"][:J], t["t"][:J] = sg, tt
        pts = P[f * consume + 1:(f + 1) * consume + 1]
        out.append({"x0": P[f * consume, :, 0].copy(), "y0": P[f * consume, :, 1].copy(), "yaw": yaw,
                    "px": np.ascontiguousarray(pts[..., 0]), "py": np.ascontiguousarray(pts[..., 1]),
                    "n_out": np.full(P.shape[1], consume if n_out is None else n_out, np.int32),
                    "traffic": t, "consume": consume})
    return out


def ramp_speeds(up=60, ramp=30, down=25):
    """From rest at 5.5 m/s^2 for `up` steps, then the acceleration falls to -5.5 over `ramp` steps and
    stays for `down`: |a| <= 5.5, under 8 m/s, windowed jerk -11 m/s^3 from step up + ramp + 10 to up + 50."""
    a = np.concatenate([np.full(up, 5.5), np.linspace(5.5, -5.5, ramp + 1)[1:], np.full(down, -5.5)])
    return np.cumsum(a * DT)


def hand_cases(geo, S):
    """name -> (frames, cfg overrides): the issue's hand-made frames, one frame each."""
    seg1 = base_segment(geo, 1)[0]
    far = (seg1 + 40) % geo.n
    out = {}
    P, yaw = track(geo, S, 0.08 * np.arange(1, 101))                       # 4 m/s^2 from rest
    parked = cars_on(geo, S, [(0, far, 3.0, 0.0, 10.0), (1, seg1, 14.5, 0.0, 0.0)])   # car 1: 9.5 m ahead of scene 0
    out["collision"] = frames_of(geo, P, yaw, parked, 100)
    one = cars_on(geo, S, [(0, far, 3.0, 0.1, 12.0)])
    out["speed"] = frames_of(geo, *track(geo, S, np.full(60, 23.0)), one, 60)
    out["acc_step"] = frames_of(geo, *track(geo, S, np.concatenate([np.zeros(5), np.full(25, 15.0)])), one, 30)
    out["jerk_ramp"] = frames_of(geo, *track(geo, S, ramp_speeds()), one, 115)
    out["off_lane"] = frames_of(geo, *track(geo, S, 0.04 * np.arange(1, 161), lane=geo.NL - 1, lat=1.5), one, 160)
    out["clean"] = frames_of(geo, *track(geo, S, 0.08 * np.arange(1, 91)), one, 90)
    return out


def wrap_frames(geo, S, consume, parked=False, steps=90):
    """90 steps (more than the 64-entry ring) of a jerk ramp (-11 m/s^3 at steps 70 to 90), 1.2 m right of lane 1's centre (off
    every lane, still in the way of lane 1's cars), among 12 cars on the same stretch."""
    seg1 = base_segment(geo, 1)[0]
    rows = [(j % geo.NL, seg1, 2.0 + 2.5 * j, 0.1 * (j % 3 - 1), 0.0 if parked else 1.0 + 0.7 * j) for j in range(12)]
    P, yaw = track(geo, S, ramp_speeds(40, 20, 30)[:steps], lat=1.2)
    return frames_of(geo, P, yaw, cars_on(geo, S, rows), consume)


WRAP_CFG = {"off_lane_steps": 40}


def run_lib(m, frames, cfg, dev=None, judge=None):
    """The library over `frames`: the host twin (dev None) or pp_judge_frame on torch device `dev`."""
    S = len(frames[0]["x0"])
    xp = "numpy" if dev is None else "torch"
    if judge is None:
        judge = ppamd.alloc_judge(S, xp=xp, device=dev)
    for fr in frames:
        sc = ppamd.alloc_scenes(S, 1)
        sc["ego_x"], sc["ego_y"], sc["ego_yaw_deg"] = fr["x0"], fr["y0"], np.ascontiguousarray(fr["yaw"], np.float64)
        res = {"n_out": fr["n_out"], "next_x": fr["px"], "next_y": fr["py"]}
        tr = fr["traffic"]
        if dev is not None:
            sc, res, tr = ({k: up(v, dev) for k, v in d.items()} for d in (sc, res, tr))
        ppamd.judge_frame(m, sc, tr, res, judge, consume=fr["consume"], cfg=cfg, host=dev is None)
    if dev is not None:
        import torch
        torch.cuda.synchronize()
    return ppamd.judge_to_numpy(judge)


def run_oracle(geo, frames, cfg):
    o = Oracle(geo, len(frames[0]["x0"]), cfg)
    for fr in frames:
        o.frame(fr["x0"], fr["y0"], fr["yaw"], fr["px"], fr["py"], fr["n_out"], fr["traffic"], fr["consume"])
    return o


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    return {"m": m, "wx": wx, "wy": wy, "geo": Geo(m.geometry())}


# ---- CPU: the host twin against the oracle -------------------------------------------------------
HAND = ["collision", "speed", "acc_step", "jerk_ramp", "off_lane", "clean"]


@pytest.fixture(scope="module")
def hand(cpu):
    S = 5
    cfg = ppamd.default_judge_cfg()
    cases = hand_cases(cpu["geo"], S)
    return {k: (cases[k], run_lib(cpu["m"], cases[k], cfg), run_oracle(cpu["geo"], cases[k], cfg)) for k in HAND}


@pytest.mark.parametrize("name", HAND)
def test_hand_made_frames_vs_oracle(hand, name):
    _, got, o = hand[name]
    compare(got, o, hand=True)


def test_hand_made_expectations(hand):
    """Scene 0 of every hand-made frame against figures worked out from its inputs."""
    fr, got, _ = hand["collision"]
    P = np.concatenate([fr[0]["x0"][None, :1], fr[0]["px"][:, :1]])
    Q = np.concatenate([fr[0]["y0"][None, :1], fr[0]["py"][:, :1]])
    driven = np.sqrt((P - P[0]) ** 2 + (Q - Q[0]) ** 2)[:, 0]
    step = int(np.argmax(driven >= 9.5 - 4.5))       # two 4.5 m cars in line touch at a 4.5 m centre gap
    assert step == 79 and abs(driven[step] - 5.0) > 1e-3
    assert got["first_step"][COL, 0] == step and got["first_car"][0] == 2
    assert got["count"][COL, 0] == 100 - step + 1 and got["flags"][0] == ppamd.INC_COLLISION
    assert abs(got["clean_dist"][0] - driven[step - 1]) <= TOL and abs(got["dist"][0] - driven[100]) <= TOL
    _, got, _ = hand["speed"]
    assert got["flags"][0] & ppamd.INC_SPEED and got["first_step"][SPD, 0] == 1 and got["count"][SPD, 0] == 60
    assert abs(got["max_speed_mph"][0] - 23 * 2.237) <= TOL
    _, got, _ = hand["acc_step"]
    assert got["flags"][0] == ppamd.INC_ACC
    assert got["first_step"][ACC, 0] == 10 and got["count"][ACC, 0] == 6 and abs(got["max_acc"][0] - 75.0) <= TOL
    _, got, _ = hand["jerk_ramp"]
    assert got["flags"][0] == ppamd.INC_JERK
    assert 90 <= got["first_step"][JRK, 0] <= 100 and abs(got["max_jerk"][0] - 11.0) <= 1e-6
    assert got["max_acc"][0] <= 5.5 + 1e-6
    _, got, _ = hand["off_lane"]
    assert got["flags"][0] == ppamd.INC_OFF_LANE
    assert got["first_step"][OFF, 0] == 151 and got["count"][OFF, 0] == 10 and got["off_run"][0] == 160
    _, got, _ = hand["clean"]
    assert not got["flags"].any() and not got["count"].any() and not got["first_step"].any()
    np.testing.assert_array_equal(got["clean_dist"], got["dist"])
    assert got["dist"][0] > 6.0


def test_plan_shorter_than_consume(cpu):
    """n_out of 0, 1 and 2 with consume 3, two frames: the ego stands still once the plan runs out,
    and the zeros beyond n_out are never read."""
    geo, S = cpu["geo"], 3
    P, yaw = track(geo, S, 0.08 * np.arange(1, 7))
    tr = cars_on(geo, S, [(1, base_segment(geo, 1)[0], 9.0, 0.0, 2.0)])
    frames = frames_of(geo, P, yaw, tr, 3)
    for f, fr in enumerate(frames):
        fr["n_out"] = np.arange(S, dtype=np.int32)
        for s in range(S):
            fr["px"][s:, s] = 0.0
            fr["py"][s:, s] = 0.0
            if f:                  # the ego is where the first frame left it
                k = int(frames[0]["n_out"][s])
                fr["x0"][s], fr["y0"][s] = (frames[0]["px"][k - 1, s], frames[0]["py"][k - 1, s]) if k else \
                    (frames[0]["x0"][s], frames[0]["y0"][s])
    cfg = ppamd.default_judge_cfg()
    got = run_lib(cpu["m"], frames, cfg)
    compare(got, run_oracle(geo, frames, cfg), hand=True)
    assert got["dist"][0] == 0.0 and not (got["flags"] & ppamd.INC_SPEED).any()


@pytest.mark.parametrize("n_cars", [0, 1, 12, 100])
def test_car_counts(cpu, n_cars):
    geo, S = cpu["geo"], 4
    seg1 = base_segment(geo, 1)[0]
    rows = [(j % geo.NL, seg1, 2.0 + 0.9 * j, 0.1 * (j % 3 - 1), 1.0 + 0.05 * j) for j in range(n_cars)]
    frames = frames_of(geo, *track(geo, S, ramp_speeds()[:30]), cars_on(geo, S, rows), 3)
    cfg = ppamd.default_judge_cfg()
    got = run_lib(cpu["m"], frames, cfg)
    compare(got, run_oracle(geo, frames, cfg), hand=True)
    assert np.isinf(got["min_sep"]).all() == (n_cars == 0)
    if n_cars >= 12:
        assert (got["flags"] & ppamd.INC_COLLISION).all()


@pytest.mark.parametrize("consume", [1, 3, 7])
def test_consume_counts(cpu, consume):
    geo, S = cpu["geo"], 4
    frames = wrap_frames(geo, S, consume, steps=21)
    cfg = ppamd.default_judge_cfg(**WRAP_CFG)
    compare(run_lib(cpu["m"], frames, cfg), run_oracle(geo, frames, cfg), hand=True)


def test_ring_wrap(cpu):
    """30 frames x consume 3 = 90 steps: the velocity ring wraps, and the segment hint and the
    off-lane run are carried over frames (off_lane_steps 40: OFF_LANE from step 41)."""
    geo = cpu["geo"]
    frames = wrap_frames(geo, 6, 3)
    cfg = ppamd.default_judge_cfg(**WRAP_CFG)
    got = run_lib(cpu["m"], frames, cfg)
    compare(got, run_oracle(geo, frames, cfg))
    assert (got["first_step"][OFF] == 41).all() and (got["count"][OFF] == 50).all()
    assert (got["flags"] & ppamd.INC_JERK).all() and (got["flags"] & ppamd.INC_COLLISION).all()


def test_split_calls_identical_bits(cpu):
    """The same 90 steps as 90 calls of consume 1 (parked cars: one advance from the frame's start
    has the bits of any split): every field of the state bit for bit."""
    geo = cpu["geo"]
    cfg = ppamd.default_judge_cfg(**WRAP_CFG)
    a = run_lib(cpu["m"], wrap_frames(geo, 6, 3, parked=True), cfg)
    b = run_lib(cpu["m"], wrap_frames(geo, 6, 1, parked=True), cfg)
    same_bits(a, b)
    assert (a["flags"] & ppamd.INC_COLLISION).any() and (a["steps"] == 90).all()


def test_reused_state_restarts_from_zero_steps(cpu):
    """A used state whose `steps` alone is zeroed judges a new episode like a zero-filled one (100
    steps: every ring entry is written again)."""
    geo = cpu["geo"]
    cfg = ppamd.default_judge_cfg(**WRAP_CFG)
    used = ppamd.alloc_judge(6)
    run_lib(cpu["m"], wrap_frames(geo, 6, 3), cfg, judge=used)
    used["steps"][:] = 0
    frames = hand_cases(geo, 6)["collision"]
    a = run_lib(cpu["m"], frames, cfg, judge=used)
    b = run_lib(cpu["m"], frames, cfg)
    same_bits(a, b)


def closed_loop_cpu(cpu, S, F, seed):
    """oracle_rollout one frame at a time on dense 100-car traffic; the host twin and the oracle judge
    every frame from the pre-frame state and the frame's plan. Scene 0 is made to drive clean: its ego
    starts at rest with no previous path (v_0 = 0 is then true, and its first plan starts at the ego,
    not nine points behind it as the synthetic scenes' do), and its cars start half a loop away."""
    olib = oracle_lib.load_oracle()
    sc, tr = many_car_traffic(cpu["m"], S, seed, dense=True)
    sc["ego_speed_mph"][0], sc["n_prev"][0], sc["n_cars"][0] = 0.0, 0, 0
    sc["prev_x"][:, 0], sc["prev_y"][:, 0] = 0.0, 0.0
    tr["seg"][:, 0] = (tr["seg"][:, 0] + cpu["geo"].n // 2) % cpu["geo"].n
    prm = ppamd.default_params(n_speeds=1)
    cfg = ppamd.default_judge_cfg()
    judge = ppamd.alloc_judge(S)
    o = Oracle(cpu["geo"], S, cfg)
    for f in range(F):
        pre_sc, pre_tr = oracle_lib.copy_state(sc, tr)
        lg = oracle_lib.oracle_rollout(olib, cpu["wx"], cpu["wy"], sc, tr, prm, 1, 3, 400.0)
        res = {"n_out": np.ascontiguousarray(lg["n_out"][0]), "next_x": np.ascontiguousarray(lg["plan_x"][0]),
               "next_y": np.ascontiguousarray(lg["plan_y"][0])}
        ppamd.judge_frame(cpu["m"], pre_sc, pre_tr, res, judge, consume=3, cfg=cfg)
        o.frame(pre_sc["ego_x"], pre_sc["ego_y"], pre_sc["ego_yaw_deg"], res["next_x"], res["next_y"], res["n_out"],
                pre_tr, 3)
    return ppamd.judge_to_numpy(judge), o


def test_closed_loop_cpu(cpu):
    """16 scenes x 150 frames of the planner in dense traffic: scene 0 (built to) stays clean while it
    speeds up from rest, the scenes in the traffic collide, and every record agrees with the oracle."""
    got, o = closed_loop_cpu(cpu, 16, 150, 23)
    compare(got, o)
    assert (got["flags"][1:] & ppamd.INC_COLLISION).any(), got["flags"]
    assert got["flags"][0] == 0 and got["dist"][0] > 50.0, (got["flags"], got["dist"][0])
    clean = got["flags"] == 0
    np.testing.assert_array_equal(got["clean_dist"][clean], got["dist"][clean])
    assert (got["clean_dist"][~clean] < got["dist"][~clean]).all()


def test_argument_errors(cpu):
    geo = cpu["geo"]
    fr = hand_cases(geo, 2)["clean"][0]
    sc = ppamd.alloc_scenes(2, 1)
    sc["ego_x"], sc["ego_y"], sc["ego_yaw_deg"] = fr["x0"], fr["y0"], np.ascontiguousarray(fr["yaw"])
    b, T = ppamd.scene_struct(sc), ppamd.traffic_struct(fr["traffic"])
    R = ppamd.result_struct({"n_out": fr["n_out"], "next_x": fr["px"], "next_y": fr["py"]})
    judge = ppamd.alloc_judge(2)
    J = ppamd.judge_struct(judge)

    def call(cfg, consume=3, state=J, host=True):
        st = C.byref(state) if state is not None else None
        if host:
            return ppamd.lib.pp_judge_frame_host(cpu["m"].handle, C.byref(b), C.byref(T), C.byref(R), consume,
                                                 C.byref(cfg), st)
        return ppamd.lib.pp_judge_frame(cpu["m"].handle, C.byref(b), C.byref(T), C.byref(R), consume, C.byref(cfg),
                                        st, 0, None)

    ok = ppamd.default_judge_cfg()
    assert (ok.speed_limit_mph, ok.max_acc, ok.max_jerk, ok.acc_window, ok.jerk_window) == (50, 10, 10, 10, 50)
    assert (ok.ego_length, ok.car_length, ok.ego_width, ok.car_width, ok.lane_tol, ok.off_lane_steps) == \
        (4.5, 4.5, 2.0, 2.0, 1.0, 150)
    for host in (True, False):       # every check comes before any HIP call
        assert call(ppamd.default_judge_cfg(acc_window=14, jerk_window=50), host=host) == -1    # Wa + Wj > 63
        assert call(ppamd.default_judge_cfg(acc_window=0), host=host) == -1
        assert call(ppamd.default_judge_cfg(jerk_window=0), host=host) == -1
        assert call(ok, state=None, host=host) == -1
        assert call(ok, consume=0, host=host) == -1
        holed = ppamd.judge_struct(judge)
        holed.ring_vy = None
        assert call(ok, state=holed, host=host) == -1
    assert not judge["steps"].any()
    assert call(ppamd.default_judge_cfg(acc_window=13, jerk_window=50)) == 0                    # Wa + Wj = 63
    prm = ppamd.default_params(n_speeds=1)
    rc = ppamd.RolloutCfg(1, 3, 100.0)
    assert ppamd.lib.pp_rollout_judged(cpu["m"].handle, C.byref(b), C.byref(T), C.byref(prm), C.byref(rc), C.byref(R),
                                       None, 0, None, C.byref(ok), None) == -1


def test_four_lane_build_host():
    """The 4-lane library's host twin judges all four lanes (tests/judge_lanes4_cases.py, a child
    process: a process loads one PP_NUM_LANES)."""
    run_lanes4("judge_lanes4_cases.py", "not gpu")


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
class TestJudgeGPU:
    @pytest.fixture(scope="class")
    def env(self, cpu):
        import torch
        return dict(cpu, torch=torch, dev=torch.device("cuda", 0))

    @pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
    def test_device_equals_host_twin_bit_for_bit(self, env, S):
        cfg = ppamd.default_judge_cfg()
        for name, frames in hand_cases(env["geo"], S).items():
            same_bits(run_lib(env["m"], frames, cfg, dev=env["dev"]), run_lib(env["m"], frames, cfg), name)

    def test_ring_wrap_and_split_calls_on_device(self, env):
        geo, S = env["geo"], 70
        cfg = ppamd.default_judge_cfg(**WRAP_CFG)
        frames = wrap_frames(geo, S, 3)
        got = run_lib(env["m"], frames, cfg, dev=env["dev"])
        same_bits(got, run_lib(env["m"], frames, cfg), "wrap")
        compare(got, run_oracle(geo, frames, cfg))
        a = run_lib(env["m"], wrap_frames(geo, S, 3, parked=True), cfg, dev=env["dev"])
        b = run_lib(env["m"], wrap_frames(geo, S, 1, parked=True), cfg, dev=env["dev"])
        same_bits(a, b, "split")
        assert (a["steps"] == 90).all() and (a["flags"] & ppamd.INC_COLLISION).any()

    def test_rollout_judged_disturbs_nothing_and_matches_oracle(self, env):
        """pp_rollout_judged against pp_rollout from the same start: scenes, traffic, result and the
        full log bit for bit; the judge state against the oracle replayed over the log and the
        start traffic (advanced by arc length)."""
        t, dev = env["torch"], env["dev"]
        S, F, consume = 384, 40, 3
        prm = ppamd.default_params(n_speeds=1)
        cfg = ppamd.default_judge_cfg()
        runs = []
        for judged in (False, True):
            d, g = ppamd.synth_traffic(env["m"], S, seed=11, device=0)
            t.cuda.synchronize()
            start = ({k: x.cpu().numpy() for k, x in d.items()},
                     {k: (x.cpu().numpy() if isinstance(x, t.Tensor) else x) for k, x in g.items()})
            res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
            lg = ppamd.alloc_log(F, S, 50, xp="torch", device=dev)
            judge = ppamd.alloc_judge(S, xp="torch", device=dev)
            if judged:
                ppamd.rollout_judged(env["m"], d, g, prm, res, judge, F, consume, 100.0, lg, cfg=cfg)
            else:
                ppamd.rollout(env["m"], d, g, prm, res, F, consume, 100.0, lg)
            t.cuda.synchronize()
            runs.append([{k: x.cpu().numpy() for k, x in dd.items() if isinstance(x, t.Tensor)}
                         for dd in (d, g, res, lg)] + [ppamd.judge_to_numpy(judge), start])
        for what, a, b in zip(("scenes", "traffic", "result", "log"), runs[0], runs[1]):
            same_bits(a, b, what)
        assert not runs[0][4]["steps"].any()
        lg, got, (sc0, tr0) = runs[1][3], runs[1][4], runs[1][5]
        geo = env["geo"]
        o = Oracle(geo, S, cfg)
        J = tr0["n_cars"]
        for f in range(F):
            tr = dict(tr0)
            tr["seg"], tr["t"] = geo.place(tr0["lane"][:J], tr0["seg"][:J], tr0["t"][:J],
                                           tr0["speed"][:J] * DT * consume * f)
            o.frame(lg["ego_x"][f], lg["ego_y"][f], sc0["ego_yaw_deg"], lg["plan_x"][f], lg["plan_y"][f],
                    lg["n_out"][f], tr, consume)
        compare(got, o)
        assert (got["steps"] == F * consume).all() and np.isfinite(got["min_sep"]).all()

    def test_dense_traffic_device_equals_host_frame_by_frame(self, env):
        """Dense 100-car traffic, 64 scenes x 150 frames of pp_rollout_judged, one frame per call; the
        host twin judges every frame from the GPU's own pre-frame state and plan: every field of the
        state bit for bit, and collisions are seen."""
        t, dev = env["torch"], env["dev"]
        S, F = 64, 150
        sc, tr = many_car_traffic(env["m"], S, 23, dense=True)
        d = {k: up(v, dev) for k, v in sc.items()}
        g = {k: up(v, dev) for k, v in tr.items()}
        prm = ppamd.default_params(n_speeds=1)
        cfg = ppamd.default_judge_cfg()
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        host = ppamd.alloc_judge(S)
        for f in range(F):
            pre_sc = {k: d[k].cpu().numpy() for k in d}
            pre_tr = {k: (x.cpu().numpy() if isinstance(x, t.Tensor) else x) for k, x in g.items()}
            ppamd.rollout_judged(env["m"], d, g, prm, res, judge, 1, 3, 400.0, cfg=cfg)
            t.cuda.synchronize()
            plan = {k: res[k].cpu().numpy() for k in ("n_out", "next_x", "next_y")}
            ppamd.judge_frame(env["m"], pre_sc, pre_tr, plan, host, consume=3, cfg=cfg)
        got = ppamd.judge_to_numpy(judge)
        same_bits(got, ppamd.judge_to_numpy(host), "dense")
        ncol = int(((got["flags"] & ppamd.INC_COLLISION) != 0).sum())
        print(f"dense 100 cars: {S} scenes x {F} frames, {ncol} scenes collided, "
              f"{int((got['flags'] == 0).sum())} clean")
        assert ncol >= 1

    def test_four_lane_build_device(self):
        run_lanes4("judge_lanes4_cases.py", "gpu")
