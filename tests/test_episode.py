"""Episode starts (include/pp.h pp_synth_episode; csrc/pp_episode.h): seeded start states made to be
driven and judged — the previous path ahead of the ego, traffic placed at the car-following rule's
gaps, a warm judge state, a reset follow state.

The definitions are the project's own (DESIGN.md "Episode starts"). Nothing restates the random
stream: every claim is recomputed from the generator's outputs with NumPy, arcs from world_lib.Geo
(a cumulative sum over pp_map_geometry's polylines, not the library's walk), the required gap from the
formula of DESIGN.md §15 written out below. Tolerances: positions within 1e-9 m (coordinates up to
3e3 m carry 5e-13 m per operation; a walk adds at most 181 roundings of an arc up to 7e3 m, 2e-10 m);
the gap's lower bound is exact (gap_slack = 1e-6 m is what covers those roundings), its upper bound
has 1e-6 m of room as the issue sets it.

Step numbers: a warm judge state starts at steps = PP_JUDGE_RING, so driven step k of the episode is
first_step = PP_JUDGE_RING + k."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import DT, MPH, Geo, run_lanes4, same_bits, to_np

RING = ppamd.JUDGE_RING
SEED = 20261020
# SHA-256 of pp_synth_traffic_host(seed 7, scenes 0..299): every scene and table array in name order,
# then the traffic's lane, seg, t, offset, speed; recorded from the commit before this generator
PARENT_SHA = "e382434fcd0a55ec323b31bcf9275b4f8a0a785a413fdf366f5dcfab844db6d4"


def fdict(cfg):
    return {k: getattr(cfg, k) for k, _ in ppamd.FollowCfg._fields_}


def req(c, vf, vl):
    """§15's s*: the net gap a follower at vf needs behind a leader at vl."""
    return c["min_gap"] + np.maximum(0.0, vf * c["time_headway"] + vf * (vf - vl) / (2 * np.sqrt(c["max_acc"] * c["comfort_brake"])))


def make(m, S, seed=SEED, first=0, cfg=None, fcfg=None, states=True):
    """Host start: (scenes, traffic, judge, follow)."""
    cfg = cfg if cfg is not None else ppamd.default_episode_cfg()
    judge = ppamd.alloc_judge(S) if states else None
    follow = ppamd.alloc_follow(S, max(cfg.n_cars, 1)) if states else None
    sc, tr = ppamd.synth_episode_host(m, S, seed, first, cfg, fcfg, judge=judge, follow=follow)
    return sc, tr, judge, follow


def state_bytes(sc, tr):
    h = hashlib.sha256()
    for k in sorted(sc):
        h.update(np.ascontiguousarray(sc[k]).tobytes())
    for k in ("lane", "seg", "t", "offset", "speed"):
        h.update(np.ascontiguousarray(tr[k]).tobytes())
    return h.hexdigest()


def ego_place(geo, sc):
    """(lane, seg, t, distance) of the ego: the nearest point over every segment of every lane."""
    p = np.stack([sc["ego_x"], sc["ego_y"]], -1)
    ap = p[None, :, None, :] - geo.A[:, None]                                      # [NL, S, n, 2]
    tt = np.clip((ap * geo.D[:, None]).sum(-1) / (geo.D ** 2).sum(-1)[:, None], 0.0, 1.0)
    q = ap - geo.D[:, None] * tt[..., None]
    d = np.sqrt((q ** 2).sum(-1))                                                  # [NL, S, n]
    S = p.shape[0]
    flat = d.transpose(1, 0, 2).reshape(S, -1)
    k = flat.argmin(1)
    lane, seg = k // geo.n, k % geo.n
    s = np.arange(S)
    return lane, seg, tt[lane, s, seg], d[lane, s, seg]


def ego_on(geo, sc, judge):
    """(lane, seg, t) of the ego as the generator placed it: the nearest lane, the judge state's segment
    (a point on a waypoint belongs to two) and the fraction of the ego's point on that segment."""
    lane = ego_place(geo, sc)[0]
    own = ppamd.judge_to_numpy(judge)["seg_hint"]
    p = np.stack([sc["ego_x"], sc["ego_y"]], -1)
    A, D = geo.A[lane, own], geo.D[lane, own]
    return lane, own, ((p - A) * D).sum(-1) / (D ** 2).sum(-1)


def rel_arcs(geo, sc, tr, seg_e, t_e):
    """Arc of every car round its lane's ring from the ego's (seg, t) on that lane: [J, S] in [0, loop)."""
    J = tr["n_cars"]
    lane = tr["lane"][:J]
    arc_c = geo.cum0[lane, tr["seg"][:J]] + tr["t"][:J] * geo.L[lane, tr["seg"][:J]]
    arc_e = geo.cum0[lane, seg_e[None]] + t_e[None] * geo.L[lane, seg_e[None]]
    return np.mod(arc_c - arc_e, geo.tot[lane])


# ---- the checks, shared with the four-lane cases ------------------------------------------------------
def check_invariants(geo, sc, tr, judge, cfg):
    S, J = len(sc["ego_x"]), cfg.n_cars
    assert tr["n_cars"] == J
    lane, seg, t, dist = ego_place(geo, sc)
    assert dist.max() <= 1e-9, dist.max()
    # a point on a waypoint belongs to two segments: the generator's own segment must be as near
    _, own, t = ego_on(geo, sc, judge)
    assert ((t >= 0) & (t < 1)).all()
    u = geo.U[lane, own]
    on_own = np.abs(((np.stack([sc["ego_x"], sc["ego_y"]], -1) - geo.A[lane, own]) * np.stack([u[:, 1], -u[:, 0]], -1)).sum(-1))
    assert on_own.max() <= 1e-9
    np.testing.assert_array_equal(sc["prev_target_lane"], lane)
    yaw = np.degrees(np.arctan2(u[:, 1], u[:, 0]))
    assert np.abs(sc["ego_yaw_deg"] - yaw).max() <= 1e-9
    ve = sc["ego_speed_mph"] / MPH
    assert (ve >= cfg.ego_speed_min - 1e-12).all() and (ve <= cfg.ego_speed_max + 1e-12).all()
    if cfg.ego_speed_max > cfg.ego_speed_min:
        assert ve.std() > 0.1 * (cfg.ego_speed_max - cfg.ego_speed_min)
    np.testing.assert_array_equal(sc["n_prev"], np.where(ve > 0, 10, 0))
    p = np.stack([sc["ego_x"], sc["ego_y"]], -1)
    for k in range(10):
        want = p + ((k + 1) * (ve * DT))[:, None] * u
        assert np.abs(sc["prev_x"][k] - want[:, 0]).max() <= 1e-9 and np.abs(sc["prev_y"][k] - want[:, 1]).max() <= 1e-9
    # rows
    np.testing.assert_array_equal(sc["n_cars"], np.full(S, J))
    if J:
        np.testing.assert_array_equal(sc["car_id"][:J], np.broadcast_to(np.arange(J)[:, None], (J, S)))
        c, cu = geo.car(tr["lane"][:J], tr["seg"][:J], tr["t"][:J], tr["offset"][:J])
        assert np.abs(sc["car_x"][:J] - c[..., 0]).max() <= 1e-9 and np.abs(sc["car_y"][:J] - c[..., 1]).max() <= 1e-9
        v = tr["speed"][:J]
        assert np.abs(sc["car_vx"][:J] - cu[..., 0] * v).max() <= 1e-9
        assert np.abs(sc["car_vy"][:J] - cu[..., 1] * v).max() <= 1e-9
        assert (v >= cfg.car_speed_min).all() and (v <= cfg.car_speed_max).all()
        assert (np.abs(tr["offset"][:J]) <= cfg.offset_jitter).all()
        assert ((tr["t"][:J] >= 0) & (tr["t"][:J] <= 1)).all()
        assert ((tr["seg"][:J] >= 0) & (tr["seg"][:J] < geo.n)).all()
    assert not sc["tab_valid"].any()
    np.testing.assert_array_equal(sc["tab_id"], np.broadcast_to(np.arange(sc["tab_id"].shape[0])[:, None], sc["tab_id"].shape))
    # statistics
    rel = rel_arcs(geo, sc, tr, own, t)
    ahead = rel < geo.tot[tr["lane"][:J]] / 2
    share = ahead.mean()
    f_car = np.bincount(tr["lane"][:J].ravel(), minlength=geo.NL) / (J * S)
    f_ego = np.bincount(lane, minlength=geo.NL) / S
    print(f"episode invariants: {S} scenes x {J} cars, ahead share {share:.4f}, car lanes {f_car.round(3).tolist()}, "
          f"ego lanes {f_ego.round(3).tolist()}")
    assert 0.70 <= share <= 0.80, share
    if geo.NL == 3:
        assert ((f_car >= 0.25) & (f_car <= 0.42)).all() and ((f_ego >= 0.25) & (f_ego <= 0.42)).all()
    else:
        assert (f_car > 0).all() and (f_ego > 0).all()
    return lane, own, t


def check_gaps(geo, sc, tr, own, t, cfg, c):
    """Per scene and lane, the ego counted on every lane: every neighbouring pair round the ring keeps
    at least req(follower, leader); every pair but the one where the front-most car faces the
    back-most keeps less than req + gap_slack + extra_gap + 1e-6."""
    S, J = len(sc["ego_x"]), tr["n_cars"]
    rel = rel_arcs(geo, sc, tr, own, t)
    ve = sc["ego_speed_mph"] / MPH
    pairs, worst = 0, np.inf
    for s in range(S):
        for l in range(geo.NL):
            on = np.nonzero(tr["lane"][:J, s] == l)[0]
            if not len(on):
                continue
            order = on[np.argsort(rel[on, s])]
            a = np.concatenate([[0.0], rel[order, s]])
            v = np.concatenate([[ve[s]], tr["speed"][order, s]])
            ln = np.concatenate([[c["ego_length"]], np.full(len(order), c["car_length"])])
            nxt = np.roll(np.arange(len(a)), -1)
            centre = np.mod(a[nxt] - a, geo.tot[l])
            net = centre - (ln + ln[nxt]) / 2
            need = req(c, v, v[nxt])
            assert (net >= need).all(), (s, l, net - need)
            wide = net >= need + cfg.gap_slack + cfg.extra_gap + 1e-6
            assert wide.sum() <= 1, (s, l, net - need)
            pairs += len(a)
            worst = min(worst, float((net - need).min()))
    print(f"episode gaps: {pairs} neighbouring pairs, smallest margin over the required gap {worst:.3e} m")
    return pairs


def check_first_follow(m, geo, sc, tr, own, t, lane, cfg, c, fcfg=None):
    """One follow update from the start: nobody brakes harder than max_acc (g >= s* and v = v0 make
    a >= -max_acc); the first car behind the ego in its lane follows the ego (where the follow rule
    sees it at all: a net gap within the horizon)."""
    S, J = len(sc["ego_x"]), tr["n_cars"]
    follow = ppamd.alloc_follow(S, max(J, 1))
    t2 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in tr.items()}
    ppamd.traffic_follow(m, sc, t2, follow, consume=3, cfg=fcfg)
    acc = (t2["speed"][:J] - tr["speed"][:J]) / (3 * DT)
    print(f"episode first follow update: hardest braking {acc.min():.5f} m/s^2")
    assert (acc >= -c["max_acc"] - 1e-9).all(), acc.min()
    rel = rel_arcs(geo, sc, tr, own, t)
    loop = geo.tot[tr["lane"][:J]]
    behind = (tr["lane"][:J] == lane[None]) & (rel >= loop / 2)
    back = np.where(behind, loop - rel, np.inf)                      # centre distance behind the ego
    j = back.argmin(0)
    has = np.isfinite(back.min(0))
    gap = back.min(0) - (c["car_length"] + c["ego_length"]) / 2
    seen = has & (gap <= c["horizon"] - 1e-6)
    lead = follow["leader"][j, np.arange(S)]
    assert seen.sum() >= S // 8, seen.sum()
    assert (lead[seen] == J).all()
    assert (lead[has & (gap > c["horizon"] + 1e-6)] == -1).all()


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    return {"m": m, "wx": wx, "wy": wy, "geo": Geo(m.geometry())}


@pytest.fixture(scope="module")
def big(cpu):
    """The default start at S = 2,000, made once and left unchanged."""
    cfg = ppamd.default_episode_cfg()
    sc, tr, judge, follow = make(cpu["m"], 2000)
    return {"sc": sc, "tr": tr, "judge": judge, "follow": follow, "cfg": cfg, "c": fdict(ppamd.default_follow_cfg())}


# ---- 1: determinism -------------------------------------------------------------------------------------
def test_same_seed_same_bytes_and_shards_concatenate(cpu):
    m = cpu["m"]
    a = make(m, 300)
    b = make(m, 300)
    lo, hi = make(m, 120), make(m, 180, first=120)
    other = make(m, 300, seed=SEED + 1)
    for x, y, z0, z1 in zip(a, b, lo, hi):
        x = {k: v for k, v in x.items() if isinstance(v, np.ndarray)}
        same_bits(x, {k: y[k] for k in x}, "repeat")
        same_bits(x, {k: np.concatenate([z0[k], z1[k]], axis=-1) for k in x}, "shards")
    assert state_bytes(a[0], a[1]) != state_bytes(other[0], other[1])
    assert (a[0]["ego_x"] != other[0]["ego_x"]).mean() > 0.99


def test_synth_traffic_host_keeps_the_parent_commits_bytes(cpu):
    """Philox's new tag parameter defaults to the scene generator's constant: pp_synth_traffic_host draws
    what it drew before."""
    sc, tr = ppamd.synth_traffic_host(cpu["m"], 300, seed=7)
    assert state_bytes(sc, tr) == PARENT_SHA


def test_episode_stream_is_not_the_scene_generators(cpu):
    sc, _, _, _ = make(cpu["m"], 64, seed=7)
    old, _ = ppamd.synth_traffic_host(cpu["m"], 64, seed=7)
    assert (sc["ego_x"] != old["ego_x"]).all()


# ---- 2-4: what a start is ---------------------------------------------------------------------------------
def test_invariants(cpu, big):
    check_invariants(cpu["geo"], big["sc"], big["tr"], big["judge"], big["cfg"])


def test_gaps(cpu, big):
    _, own, t = ego_on(cpu["geo"], big["sc"], big["judge"])
    pairs = check_gaps(cpu["geo"], big["sc"], big["tr"], own, t, big["cfg"], big["c"])
    assert pairs > 2000 * 12


def test_first_follow_update_brakes_nobody_hard(cpu, big):
    lane, own, t = ego_on(cpu["geo"], big["sc"], big["judge"])
    check_first_follow(cpu["m"], cpu["geo"], big["sc"], big["tr"], own, t, lane, big["cfg"], big["c"])


def test_gaps_at_the_densest_default_traffic_and_another_gap_rule(cpu):
    """33 cars (the most the defaults allow: the cursors pass half the ring) and a tighter rule."""
    geo = cpu["geo"]
    for n_cars, over in ((33, {}), (20, {"time_headway": 0.6, "min_gap": 1.0, "car_length": 5.5, "ego_length": 3.5})):
        cfg = ppamd.default_episode_cfg(n_cars=n_cars)
        fcfg = ppamd.default_follow_cfg(**over)
        sc, tr, judge, _ = make(cpu["m"], 150, cfg=cfg, fcfg=fcfg)
        _, own, t = ego_on(geo, sc, judge)
        check_gaps(geo, sc, tr, own, t, cfg, fdict(fcfg))


# ---- 5: the states ------------------------------------------------------------------------------------------
def check_states(geo, sc, judge, follow):
    S = len(sc["ego_x"])
    lane = sc["prev_target_lane"]
    u = geo.U[lane, judge["seg_hint"]]
    ve = sc["ego_speed_mph"] / MPH
    j = ppamd.judge_to_numpy(judge)
    assert (j["steps"] == RING).all() and not j["flags"].any() and not j["count"].any() and not j["first_step"].any()
    assert not j["first_car"].any() and not j["off_run"].any()
    assert np.abs(j["head_x"] - u[:, 0]).max() <= 1e-12 and np.abs(j["head_y"] - u[:, 1]).max() <= 1e-12
    assert j["ring_vx"].shape == (RING, S)
    assert np.abs(j["ring_vx"] - (ve * u[:, 0])[None]).max() <= 1e-12
    assert np.abs(j["ring_vy"] - (ve * u[:, 1])[None]).max() <= 1e-12
    assert (j["ring_vx"] == j["ring_vx"][0]).all() and (j["ring_vy"] == j["ring_vy"][0]).all()
    assert np.isposinf(j["min_sep"]).all()
    for k in ("dist", "clean_dist", "max_speed_mph", "max_acc", "max_jerk"):
        assert not j[k].any(), k
    assert not follow["started"].any() and not follow["ego_seg"].any()


def test_warm_judge_state_and_reset_follow_state(cpu, big):
    check_states(cpu["geo"], big["sc"], big["judge"], big["follow"])


def test_null_states_are_accepted_and_used_states_are_reset(cpu):
    m, S = cpu["m"], 40
    want = make(m, S)
    sc, tr, _, _ = make(m, S, states=False)
    same_bits(sc, want[0], "scenes without states")
    # used states: junk everywhere, then a second call
    judge, follow = ppamd.alloc_judge(S), ppamd.alloc_follow(S, 12)
    for d in (judge, follow):
        for k, v in d.items():
            v[...] = 7
    ppamd.synth_episode_host(m, S, SEED, 0, judge=judge, follow=follow)
    same_bits(ppamd.judge_to_numpy(judge), ppamd.judge_to_numpy(want[2]), "judge")
    assert not follow["started"].any() and not follow["ego_seg"].any()
    assert (follow["desired"] == 7).all() and (follow["leader"] == 7).all()     # written by the first follow call, not here
    # either state alone
    j2 = ppamd.alloc_judge(S)
    ppamd.synth_episode_host(m, S, SEED, 0, judge=j2)
    same_bits(ppamd.judge_to_numpy(j2), ppamd.judge_to_numpy(want[2]), "judge alone")


# ---- 6: the point of the feature -----------------------------------------------------------------------------
def drive(cpu, sc, tr, judge, follow, frames, consume=3):
    """The C restatement of the planner one frame at a time with the host twins of follow and judge
    (tests/test_follow.py's drive, for any number of cars and a given judge state). Updates the state in
    place; returns the slowest traffic speed seen."""
    olib = oracle_lib.load_oracle()
    prm = ppamd.default_params(n_speeds=1)
    slowest = np.inf
    for _ in range(frames):
        ppamd.traffic_follow(cpu["m"], sc, tr, follow, consume=consume)
        slowest = min(slowest, float(tr["speed"][:tr["n_cars"]].min()))
        pre_sc, pre_tr = oracle_lib.copy_state(sc, tr)
        lg = oracle_lib.oracle_rollout(olib, cpu["wx"], cpu["wy"], sc, tr, prm, 1, consume, 400.0)
        res = {"n_out": np.ascontiguousarray(lg["n_out"][0]), "next_x": np.ascontiguousarray(lg["plan_x"][0]),
               "next_y": np.ascontiguousarray(lg["plan_y"][0])}
        ppamd.judge_frame(cpu["m"], pre_sc, pre_tr, res, judge, consume=consume)
    return slowest


def early(judge, lo=1, hi=45):
    """Scenes with a first incident of any kind at driven step lo..hi of a warm episode, and the earliest
    driven step of any incident (None: none)."""
    fs = ppamd.judge_to_numpy(judge)["first_step"] - RING
    hit = ((fs >= lo) & (fs <= hi)).any(axis=0)
    any_ = fs[fs > 0]
    return int(hit.sum()), (int(any_.min()) if len(any_) else None)


def census(judge):
    j = ppamd.judge_to_numpy(judge)
    return {k: int(((j["flags"] >> i) & 1).sum()) for i, k in enumerate(ppamd.INC_KINDS)}


@pytest.fixture(scope="module")
def drives(cpu):
    S = 256
    out = {}
    sc, tr, judge, follow = make(cpu["m"], S, seed=7)
    drive(cpu, sc, tr, judge, follow, 40)
    out["at40"] = {k: v.copy() for k, v in judge.items()}
    out["slowest"] = drive(cpu, sc, tr, judge, follow, 80)
    out["at120"] = judge
    sc, tr = ppamd.synth_traffic_host(cpu["m"], S, seed=7)
    judge, follow = ppamd.alloc_judge(S), ppamd.alloc_follow(S, 12)
    drive(cpu, sc, tr, judge, follow, 100)
    out["old"] = judge
    sc, tr, judge, follow = make(cpu["m"], S, seed=7, cfg=ppamd.default_episode_cfg(ego_speed_max=0.0))
    assert not sc["ego_speed_mph"].any() and not sc["n_prev"].any()
    drive(cpu, sc, tr, judge, follow, 40)
    out["rest"] = judge
    return out


def test_no_incident_in_the_first_45_driven_steps(drives):
    n, first = early(drives["at40"])
    print(f"episode drive, 256 scenes x 40 frames: earliest incident at driven step {first}; {census(drives['at40'])}")
    assert (ppamd.judge_to_numpy(drives["at40"])["steps"] == RING + 120).all()
    assert n == 0


def test_no_incident_in_the_first_45_driven_steps_from_rest(drives):
    n, first = early(drives["rest"])
    print(f"episode drive from rest, 256 scenes x 40 frames: earliest incident at driven step {first}; {census(drives['rest'])}")
    assert n == 0


def test_few_collisions_and_neither_speed_nor_acc_in_120_frames(drives):
    j = ppamd.judge_to_numpy(drives["at120"])
    c = census(drives["at120"])
    n, first = early(drives["at120"], 1, 360)
    print(f"episode drive, 256 scenes x 120 frames: {c}, {n} scenes with any incident, earliest at driven step {first}, "
          f"max_acc {j['max_acc'].max():.4f}, top speed {j['max_speed_mph'].max():.2f} mph, slowest car "
          f"{drives['slowest']:.2f} m/s, clean_dist median {np.median(j['clean_dist']):.1f} m")
    assert (j["steps"] == RING + 360).all()
    assert c["COLLISION"] <= 0.01 * 256
    assert c["SPEED"] == 0 and c["ACC"] == 0
    for d in (drives["at40"], drives["rest"]):
        cc = census(d)
        assert cc["SPEED"] == 0 and cc["ACC"] == 0


def test_the_benchmark_snapshot_records_incidents_nearly_everywhere(drives):
    """The same drive from pp_synth_traffic_host: what the judge said before this generator."""
    j = ppamd.judge_to_numpy(drives["old"])
    n = int((j["flags"] != 0).sum())
    print(f"drive from pp_synth_traffic_host, 256 scenes x 100 frames: {n} scenes with an incident; {census(drives['old'])}, "
          f"clean_dist median {np.median(j['clean_dist']):.1f} m")
    assert n >= 0.9 * 256
    new = ppamd.judge_to_numpy(drives["at120"])
    assert int((new["flags"] != 0).sum()) < n


# ---- 7: argument errors ---------------------------------------------------------------------------------------
def test_argument_errors(cpu):
    m, S = cpu["m"], 4
    sc = ppamd.add_car_table(ppamd.alloc_scenes(S, 40), slots=40)
    tr = ppamd.alloc_traffic(S, n=40)
    judge, follow = ppamd.alloc_judge(S), ppamd.alloc_follow(S, 40)
    b, T = ppamd.scene_struct(sc), ppamd.traffic_struct(tr)
    J, F = ppamd.judge_struct(judge), ppamd.follow_struct(follow)
    ok = ppamd.default_episode_cfg()
    assert [getattr(ok, k) for k, _ in ppamd.EpisodeCfg._fields_ if k != "_pad"] == \
        [12, 0.0, 20.0, 5.0, 25.0, 0.75, 40.0, 0.3, 1e-6]

    def ref(x):
        return C.byref(x) if x is not None else None

    def call(cfg=ok, gap=None, scenes=b, traffic=T, js=J, fs=F, host=True, handle=m.handle, first=0):
        if host:
            return ppamd.lib.pp_synth_episode_host(handle, 1, first, ref(cfg), ref(gap), ref(scenes), ref(traffic),
                                                   ref(js), ref(fs))
        return ppamd.lib.pp_synth_episode(handle, 1, first, ref(cfg), ref(gap), ref(scenes), ref(traffic), ref(js),
                                          ref(fs), 0, None)

    nan = float("nan")
    bad = [{"n_cars": -1}, {"n_cars": ppamd.MAX_CARS + 1}, {"n_cars": 41}, {"ego_speed_min": 21.0},
           {"car_speed_min": 26.0}, {"ego_speed_min": -1.0}, {"car_speed_min": -1.0}, {"ego_speed_max": nan},
           {"car_speed_max": nan}, {"ego_speed_min": nan}, {"car_speed_min": nan}, {"ahead_share": -0.1},
           {"ahead_share": 1.1}, {"ahead_share": nan}, {"extra_gap": -1.0}, {"extra_gap": nan},
           {"offset_jitter": -0.1}, {"offset_jitter": nan}, {"gap_slack": -1e-6}, {"gap_slack": nan},
           {"n_cars": 34}]
    bad_gap = [{"max_acc": 0.0}, {"comfort_brake": -1.0}, {"max_brake": 0.0}, {"gap_floor": 0.0}, {"horizon": -1.0},
               {"car_length": -0.1}, {"ego_length": nan}, {"lateral_reach": -1.0}, {"time_headway": nan}]
    for host in (True, False):           # every check comes before any HIP call: the device entry too, on a CPU box
        for over in bad:
            assert call(ppamd.default_episode_cfg(**over), host=host) == -1, over
        for over in bad_gap:
            assert call(gap=ppamd.default_follow_cfg(**over), host=host) == -1, over
        assert call(cfg=None, host=host) == -1 and call(scenes=None, host=host) == -1
        assert call(traffic=None, host=host) == -1 and call(handle=None, host=host) == -1
        assert call(first=-1, host=host) == -1
        for hole in ("ego_x", "ego_yaw_deg", "prev_y", "n_prev", "prev_target_lane", "n_cars", "car_id", "car_vy"):
            holed = ppamd.scene_struct(sc)
            setattr(holed, hole, None)
            assert call(scenes=holed, host=host) == -1, hole
        for hole in ("lane", "seg", "t", "offset", "speed"):
            holed = ppamd.traffic_struct(tr)
            setattr(holed, hole, None)
            assert call(traffic=holed, host=host) == -1, hole
        for hole in ("steps", "first_step", "ring_vy", "min_sep", "max_jerk"):
            holed = ppamd.judge_struct(judge)
            setattr(holed, hole, None)
            assert call(js=holed, host=host) == -1, hole
        for hole in ("started", "ego_seg", "desired", "gap"):
            holed = ppamd.follow_struct(follow)
            setattr(holed, hole, None)
            assert call(fs=holed, host=host) == -1, hole
        small = ppamd.scene_struct(ppamd.add_car_table(ppamd.alloc_scenes(S, 11), slots=12))
        assert call(scenes=small, host=host) == -1                       # 12 cars, 11 car columns
        small = ppamd.scene_struct(ppamd.add_car_table(ppamd.alloc_scenes(S, 12), slots=11))
        assert call(scenes=small, host=host) == -1                       # 12 cars, 11 table slots
    assert not judge["steps"].any() and not sc["n_cars"].any() and not tr["speed"].any()
    # the ring bound: 33 cars fit the defaults, 34 do not; narrower speeds make room
    assert call(ppamd.default_episode_cfg(n_cars=33)) == 0
    assert call(ppamd.default_episode_cfg(n_cars=34)) == -1
    assert call(ppamd.default_episode_cfg(n_cars=40, car_speed_max=15.0, ego_speed_max=15.0)) == 0
    # the edges that are allowed
    assert call(ppamd.default_episode_cfg(n_cars=0)) == 0
    assert call(ppamd.default_episode_cfg(ego_speed_max=0.0, ahead_share=1.0, extra_gap=0.0, offset_jitter=0.0, gap_slack=0.0)) == 0
    assert call(js=None, fs=None) == 0
    notab = ppamd.scene_struct(ppamd.alloc_scenes(S, 12))
    assert call(scenes=notab, js=None, fs=None) == 0


# ---- 8: the four-lane build -------------------------------------------------------------------------------------
def test_four_lane_build_host():
    """The 4-lane library's starts use all four lanes and keep their gaps (tests/episode_lanes4_cases.py,
    a child process: a process loads one PP_NUM_LANES)."""
    run_lanes4("episode_lanes4_cases.py", "not gpu")


# ---- GPU --------------------------------------------------------------------------------------------------------
def device_start(m, S, seed=SEED, first=0, cfg=None, dev=None):
    import torch
    cfg = cfg if cfg is not None else ppamd.default_episode_cfg()
    judge = ppamd.alloc_judge(S, xp="torch", device=dev)
    follow = ppamd.alloc_follow(S, max(cfg.n_cars, 1), xp="torch", device=dev)
    sc, tr = ppamd.synth_episode(m, S, seed, first, cfg, None, 0, None, judge=judge, follow=follow)
    torch.cuda.synchronize()
    return sc, tr, judge, follow


def device_equals_host(m, S, n_cars, first, dev):
    cfg = ppamd.default_episode_cfg(n_cars=n_cars)
    sc, tr, judge, follow = device_start(m, S, first=first, cfg=cfg, dev=dev)
    hs, ht, hj, hf = make(m, S, first=first, cfg=cfg)
    assert tr["n_cars"] == ht["n_cars"] == n_cars
    what = f"S {S} cars {n_cars} first {first}"
    same_bits(to_np(sc), hs, what + " scenes")                            # telemetry and table
    same_bits({k: v for k, v in to_np(tr).items() if k != "n_cars"}, {k: v for k, v in ht.items() if k != "n_cars"},
              what + " traffic")
    same_bits(ppamd.judge_to_numpy(judge), ppamd.judge_to_numpy(hj), what + " judge")
    same_bits(ppamd.follow_to_numpy(follow), hf, what + " follow")


@pytest.mark.gpu
class TestEpisodeGPU:
    @pytest.fixture(scope="class")
    def env(self, cpu):
        import torch
        return dict(cpu, torch=torch, dev=torch.device("cuda", 0))

    @pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
    def test_device_equals_host_bit_for_bit(self, env, S):
        for n_cars in (0, 1, 12, 33):
            device_equals_host(env["m"], S, n_cars, 0, env["dev"])

    def test_device_equals_host_beyond_32_bit_scene_indices(self, env):
        device_equals_host(env["m"], 257, 12, 2 ** 32 + 5, env["dev"])
        a = make(env["m"], 8, first=2 ** 32 + 5)[0]
        b = make(env["m"], 8, first=5)[0]
        assert (a["ego_x"] != b["ego_x"]).all()                           # the index's high word is part of the counter

    def test_rollout_reactive_from_a_device_made_start(self, env):
        t, dev = env["torch"], env["dev"]
        S, F = 256, 40
        ppamd.plan_reset(env["m"])
        sc, tr, judge, follow = device_start(env["m"], S, seed=7, dev=dev)
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        ppamd.rollout_reactive(env["m"], sc, tr, prm, res, follow, F, 3, 400.0, judge=judge)
        t.cuda.synchronize()
        j = ppamd.judge_to_numpy(judge)
        assert (j["steps"] == RING + 120).all()
        n, first = early(judge)
        c = census(judge)
        print(f"pp_rollout_reactive from pp_synth_episode, {S} scenes x {F} frames: earliest incident at driven step "
              f"{first}; {c}")
        assert n == 0
        assert c["SPEED"] == 0 and c["ACC"] == 0
        assert (ppamd.follow_to_numpy(follow)["started"] == 1).all()

    def test_four_lane_build_device(self):
        run_lanes4("episode_lanes4_cases.py", "gpu")
