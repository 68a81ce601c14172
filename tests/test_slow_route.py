"""The checked K2 route (k_prep's kLimSlow -> k_cand<true> / cand_group<true>, k_winner<true>,
k_winner_st<true>) in every mode and launch shape, with both kinds of flagged scene
(tests/slow_route_lib.py): speed-edge scenes and wound-up start headings on a ladder of magnitudes
from 9.4e4 rad (the control below kSlowAngle) to 6.3e10 rad, read by both ways start_pose has.

Contract: oracle_lib.compare's as it stands, except that a ladder scene's next_x/next_y/paths are
held to slow_route_lib.heading_bound (TOL + 0.5 ulp(|A|) n L, from the oracle's own output: the
reference accumulates its turns in a double of magnitude |A|, the library rotates (cos, sin));
below 2^24 rad that term is under 1e-6 m. Every GPU case evaluates twice back to back: under the
suite's PP_DBG_POISON the second call fails with PP_ERR_STATE if the first left a bit in the
slow-group bitmap. Every case prints the largest |dxy| per rung.

Not covered: non-finite telemetry yaw (NaN, +-inf, 1e308 degrees); DESIGN.md §5 says why."""
import contextlib

import numpy as np
import pytest

import oracle_lib
import slow_route_lib as srl
from oracle_lib import ppamd

OFFS6 = [-6, -4, -3, -2, -1]


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    return {"m": ppamd.Map(wx, wy), "wx": wx, "wy": wy, "olib": oracle_lib.load_oracle(),
            "rlib": oracle_lib.load_ref()}


@pytest.fixture(scope="module")
def ladder(cpu):
    """600 ladder scenes and the oracle's all-paths evaluation of them (shared, left unchanged)."""
    sc, meta = srl.wound_heading_scenes(cpu["m"], 600)
    prm = ppamd.default_params(emit_paths=True)
    return sc, meta, oracle_lib.oracle_eval(cpu["olib"], cpu["wx"], cpu["wy"], sc, prm, info=True)


def test_every_rung_by_both_ways(ladder):
    sc, meta, ref = ladder
    assert srl.assert_ladder_complete(meta) == 4 * len(srl.LADDER)
    assert srl.assert_ladder_complete(meta, np.arange(srl.LADDER_PERIOD)) == 4 * len(srl.LADDER)
    srl.assert_effective(ref["info"], sc, [], ladder=srl.ladder_idx(meta))
    A = np.abs(meta["A"])
    assert (A[meta["rung"] == 0] < srl.K_SLOW_ANGLE).all() and (A[meta["rung"] >= 1] > srl.K_SLOW_ANGLE).all()
    assert (A[meta["rung"] == 2] < 823549.6).all() and (A[meta["rung"] == 3] > 823549.6).all()
    assert (A[meta["rung"] == 6] < 1e8).all() and (A[meta["rung"] == 7] > 1e8).all()
    assert (meta["rung"] < 0).sum() == 200          # the ordinary third


def test_assert_effective_rejects_inert_inputs(cpu):
    """An edge speed written into a scene that keeps its previous points, and a wound yaw on a
    scene whose last step moves, are both inert: assert_effective fails on them."""
    sc = ppamd.synth_host(cpu["m"], 400, seed=24, first=72)
    idx = np.arange(2, 400, 37)
    sc["ego_speed_mph"][idx] = np.array([-0.0, 5e-324, 3e6, -3.0])[np.arange(len(idx)) % 4]
    info = oracle_lib.oracle_eval(cpu["olib"], cpu["wx"], cpu["wy"], sc, ppamd.default_params(), info=True)["info"]
    assert (sc["n_prev"][idx] == 10).any()
    with pytest.raises(AssertionError, match="do not read the telemetry speed"):
        srl.assert_effective(info, sc, idx)
    with pytest.raises(AssertionError, match="do not read the telemetry yaw"):
        srl.assert_effective(info, sc, [], ladder=idx)
    sc["n_prev"][idx] = 0
    info = oracle_lib.oracle_eval(cpu["olib"], cpu["wx"], cpu["wy"], sc, ppamd.default_params(), info=True)["info"]
    srl.assert_effective(info, sc, idx, ladder=idx)


def test_ladder_paths_are_ordinary(ladder):
    """At least 95 % of the ladder scenes have a finite, full-length oracle winner path, so no
    comparison rests on a NaN path."""
    sc, meta, ref = ladder
    lad = srl.ladder_idx(meta)
    N = ref["next_x"].shape[0]
    good = [ref["n_out"][s] == N and np.isfinite(ref["next_x"][:, s]).all() and np.isfinite(ref["next_y"][:, s]).all()
            for s in lad]
    assert np.mean(good) >= 0.95, np.mean(good)
    # the bound's extra term stays near 1e-6 m below 2^24 rad: 0.5 ulp (1.9e-9 rad) x 50 points x
    # at most 25 m (50 steps at the speed limit) = 1.2e-6 m
    b = srl.heading_bound(ref, srl.kept(sc), meta["A"])
    assert (b[(np.abs(meta["A"]) < 2.0**24)] - oracle_lib.TOL < 1.2e-6).all()
    assert (b[meta["rung"] < 0] == oracle_lib.TOL).all()


@pytest.mark.skipif(oracle_lib.load_ref() is None, reason="oracle/_ref needs the reference's sources")
def test_restatement_equals_reference_on_ladder(cpu, ladder):
    """Every candidate path and the frame's trajectory of the restatement equal the reference's own
    code bit for bit at every rung."""
    sc, meta, o = ladder
    ref = oracle_lib.ref_eval(cpu["rlib"], cpu["wx"], cpu["wy"], sc, 5, [-4.0, -2.0, 0.0, 2.0])
    op = np.transpose(o["paths"], (0, 2, 1, 3))
    same = ((op == ref["paths"]) | (np.isnan(op) & np.isnan(ref["paths"]))).reshape(len(op), -1).all(1)
    assert same.all(), (np.nonzero(~same)[0][:10], meta["rung"][~same][:10])
    assert (o["path_len"] == ref["path_len"]).all()
    assert np.array_equal(np.stack([o["next_x"].T, o["next_y"].T], -1), ref["ref_next"])
    assert (o["info"]["target_lane"] == ref["ref_T"]).all()


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    wx, wy = oracle_lib.highway_map()
    return {"torch": torch, "m": ppamd.Map(wx, wy), "wx": wx, "wy": wy,
            "olib": oracle_lib.load_oracle(), "dev": torch.device("cuda", 0)}


def to_dev(env, sc):
    return {k: env["torch"].from_numpy(np.ascontiguousarray(v)).to(env["dev"]) for k, v in sc.items()}


def same_bits(a, b, what):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), (what, k)


def ev(env, d, prm, m=None, **dbg):
    """pp_eval twice back to back with the debug switches dbg (DBG_* name without the prefix ->
    value); the two results are bit-identical; returns the first."""
    S = int(d["ego_x"].shape[0])
    rs = [ppamd.alloc_result(S, prm, xp="torch", device=env["dev"]) for _ in range(2)]
    with contextlib.ExitStack() as st:
        for k, v in dbg.items():
            st.enter_context(ppamd.debug(getattr(ppamd, "DBG_" + k), v))
        for r in rs:
            ppamd.evaluate(m or env["m"], d, prm, r, device=0)
    env["torch"].cuda.synchronize()
    a, b = (ppamd.result_to_numpy(r) for r in rs)
    same_bits(a, b, "second call")
    return a


def oracle_check(env, sc, meta, got, prm, sub=None, what="", wx=None, wy=None):
    """Scenes `sub` of the batch (default: all) against the oracle with the heading bound; every
    rung and both scene kinds present among them; prints the per-rung maxima."""
    S = sc["ego_x"].shape[0]
    sub = np.arange(S) if sub is None else np.asarray(sub)
    srl.assert_ladder_complete(meta, sub)
    part = srl.take(sc, sub)
    mc = prm.n_draws > 1
    ref = oracle_lib.oracle_eval(env["olib"], env["wx"] if wx is None else wx, env["wy"] if wy is None else wy,
                                 part, prm, info=True)
    pos = {int(s): i for i, s in enumerate(sub)}
    edge = [pos[int(s)] for s in meta.get("edge", []) if int(s) in pos]
    if "edge" in meta:
        assert len(edge) >= 4, "no speed-edge scenes in the compared subset"
    srl.assert_effective(ref["info"], part, edge, ladder=[pos[int(s)] for s in srl.ladder_idx(meta) if int(s) in pos])
    bound = srl.heading_bound(ref, srl.kept(part), meta["A"][sub])
    sel = srl.take_result(got, sub)
    if mc:
        err = srl.compare_mc_bounded(sel, ref, bound)
    else:
        err = srl.compare_bounded(sel, {k: v for k, v in ref.items() if k != "info"}, bound)
    print(f"{what}: {len(sub)} scenes, max |dxy| per rung (m): {srl.format_report(srl.rung_report(err, meta, sub))}")
    return ref


def sample(meta, S, stride=13):
    """The first 4 LADDER_PERIOD scenes of a large batch and its last LADDER_PERIOD (every rung,
    sign and way among them), a strided sample and some of the speed-edge scenes."""
    want = np.concatenate([np.arange(0, min(4 * srl.LADDER_PERIOD, S)), np.arange(max(S - srl.LADDER_PERIOD, 0), S),
                           np.arange(0, S, stride), meta.get("edge", np.array([], np.int64))[::max(1, S // 2000)]])
    return np.unique(want)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1200, 3000, 5000])
def test_reference_mode_launch_shapes(env, S):
    """Reference mode without paths, ladder and speed-edge scenes. S = 1,200: the three launch shapes,
    K1 groups 1 and 16, K1 waves 3 and 4 at group 1, all bit-identical. S = 3,000: the step's
    512-thread blocks; S = 5,000: its 16-scene blocks; each bit-identical to the three-kernel shape.
    The step's result against the oracle."""
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=20241 + S, first=S)
    d, prm = to_dev(env, sc), ppamd.default_params()
    base = ev(env, d, prm, SHAPE=ppamd.SHAPE_SPLIT)
    runs = {"step": dict(SHAPE=ppamd.SHAPE_STEP)}
    if S == 1200:
        runs.update({"cand_small": dict(SHAPE=ppamd.SHAPE_CAND_SMALL),
                     "group1": dict(SHAPE=ppamd.SHAPE_SPLIT, PREP_GROUP=1),
                     "group16": dict(SHAPE=ppamd.SHAPE_SPLIT, PREP_GROUP=16),
                     "group1_waves3": dict(SHAPE=ppamd.SHAPE_SPLIT, PREP_GROUP=1, PREP_WAVES=3),
                     "group1_waves4": dict(SHAPE=ppamd.SHAPE_SPLIT, PREP_GROUP=1, PREP_WAVES=4)})
    step = None
    for name, dbg in runs.items():
        out = ev(env, d, prm, **dbg)
        same_bits(base, out, name)
        step = out if name == "step" else step
    assert (base["status"] != 0).any()
    oracle_check(env, sc, meta, step, prm, what=f"reference mode, step, S = {S}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_speeds", [5, 6])
def test_all_paths(env, n_speeds):
    """All paths: whole scenes per group (C = 15), and the flat geometry (C = 18) whose scenes
    straddle two groups, flagged ladder scenes among the straddling ones."""
    S = 600
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=31 + n_speeds, first=600)
    prm = ppamd.default_params(emit_paths=True, n_speeds=n_speeds, speed_offsets=OFFS6 if n_speeds == 6 else None)
    if n_speeds == 6:
        C = ppamd.NUM_LANES * n_speeds
        s = np.arange(S)
        straddle = (s * C) // 256 != ((s + 1) * C - 1) // 256
        assert (straddle & (meta["rung"] >= 1)).sum() >= 10
        assert (straddle & (meta["way"] == srl.WAY_FRAME0) & (meta["rung"] >= 1)).any()
    got = ev(env, to_dev(env, sc), prm)
    oracle_check(env, sc, meta, got, prm, what=f"all paths, C = {ppamd.NUM_LANES * n_speeds}")


@pytest.mark.gpu
@pytest.mark.parametrize("emit", [False, True])
def test_comfort_mode(env, emit):
    """Comfort mode without paths (k_cand's decision, cand_store_slot<true>, k_winner_st<true>) and
    with them (k_winner<true>)."""
    S = 1500
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=77, first=1500)
    prm = ppamd.default_params(cost_mode=ppamd.COST_COMFORT, emit_paths=emit)
    got = ev(env, to_dev(env, sc), prm)
    oracle_check(env, sc, meta, got, prm, what=f"comfort mode, emit_paths = {emit}")


_DRAW0 = {}


def draw0_only(env, sc, meta, prm):
    """Scenes whose nominal draw alone holds an out-of-range speed, from the oracle's materialised
    draws: car 0 is the nominal in-lane car, its nominal speed sqrt(vx^2 + vy^2) lies in
    (0, 2^-60) (outside speed_in_range), and its speed in every noisy draw lies in [2^-60, 2^20]."""
    car = meta["car"]
    nom = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, ppamd.default_params(n_speeds=1), info=True)
    f0 = np.sqrt(sc["car_vx"][0] ** 2 + sc["car_vy"][0] ** 2)[car]
    ok = (nom["info"]["in_lane_car"][car] == sc["car_id"][0, car]) & (f0 > 0) & (f0 < 2.0**-60)
    for dr in range(1, prm.n_draws):
        nd = oracle_lib.noisy_scenes(env["olib"], sc, prm, dr)
        f = np.sqrt(nd["car_vx"][0] ** 2 + nd["car_vy"][0] ** 2)[car]
        ok &= (f >= 2.0**-60) & (f <= 2.0**20)
    return car[ok]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [ppamd.COST_REFERENCE, ppamd.COST_COMFORT])
@pytest.mark.parametrize("D,n_speeds,S", [(6, 1, 700), (24, 5, 96)])
def test_montecarlo(env, mode, D, n_speeds, S):
    """Monte-Carlo draws: several scenes per block (D = 6, C = 18) and two blocks per scene (D = 24,
    C = 360: the BPS > 1 branch of the slow-group bitmap). A scene is flagged when any of its draws
    is; the batches hold scenes flagged by draw 0 alone."""
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=400 + D, first=7 * S)
    prm = ppamd.default_params(n_speeds=n_speeds, cost_mode=mode, n_draws=D)
    if (D, S) not in _DRAW0:
        _DRAW0[(D, S)] = draw0_only(env, sc, meta, prm)
    assert len(_DRAW0[(D, S)]) >= 1, "no scene flagged by draw 0 alone"
    got = ev(env, to_dev(env, sc), prm)
    oracle_check(env, sc, meta, got, prm, what=f"Monte-Carlo mode {mode}, D = {D}, C = {ppamd.NUM_LANES * n_speeds * D} "
                                               f"({len(_DRAW0[(D, S)])} scenes flagged by draw 0 alone)")


@pytest.mark.gpu
def test_persistent_k2(env):
    """Ladder scenes strewn through (R + 5) 17 + 3 scenes: the persistent K2 against the
    one-group-per-block launch, bit-identical; the ladder scenes and a sample against the oracle."""
    import test_persist as tp
    prm = ppamd.default_params()
    tp.run(env, to_dev(env, ppamd.synth_host(env["m"], 3 * tp.SPB, seed=1, first=1)), prm, ppamd.PERSIST_ON)
    R = ppamd.debug_get(ppamd.DBG_LAST_PERSIST)
    assert R >= 1
    S = (R + 5) * tp.SPB + 3
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=55, first=S)
    d = to_dev(env, sc)
    keys = dict(SHAPE=ppamd.SHAPE_SPLIT, SPLIT=ppamd.SPLIT_OFF)
    a = ev(env, d, prm, PERSIST=ppamd.PERSIST_ON, **keys)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == R
    b = ev(env, d, prm, PERSIST=ppamd.PERSIST_OFF, **keys)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == 0
    same_bits(a, b, "persistent")
    oracle_check(env, sc, meta, a, prm, sub=sample(meta, S), what=f"persistent K2, S = {S}")


@pytest.mark.gpu
def test_forced_split(env):
    """70,013 scenes: the two-part split forced against one stream, bit-identical; the ladder
    scenes at both ends and the part boundary and a sample against the oracle."""
    S = 70013
    sc, meta = srl.mixed_slow_scenes(env["m"], S, seed=70, first=S)
    d, prm = to_dev(env, sc), ppamd.default_params()
    a = ev(env, d, prm, SPLIT=ppamd.SPLIT_ON)
    assert ppamd.debug_get(ppamd.DBG_LAST_PARTS) == 2
    b = ev(env, d, prm, SPLIT=ppamd.SPLIT_OFF)
    assert ppamd.debug_get(ppamd.DBG_LAST_PARTS) == 1
    same_bits(a, b, "split")
    sub = np.unique(np.concatenate([sample(meta, S, stride=41), np.arange(S // 2 - 150, S // 2 + 150)]))
    oracle_check(env, sc, meta, a, prm, sub=sub, what=f"forced split, S = {S}")


@pytest.mark.gpu
def test_plan_frame(env):
    """pp_plan_frame (k_plan_frame: the step body's own copy of the heading flag), one frame per
    rung, sign and way of reading the yaw, against the oracle on oracle_lib.one_scene's batch."""
    sc, meta = srl.wound_heading_scenes(env["m"], srl.LADDER_PERIOD, seed=66, first=66)
    srl.assert_ladder_complete(meta)
    prm = ppamd.default_params()
    worst = {}
    for s in srl.ladder_idx(meta):
        nc, npv = int(sc["n_cars"][s]), int(sc["n_prev"][s])
        cars = [(int(sc["car_id"][j, s]), sc["car_x"][j, s], sc["car_y"][j, s], sc["car_vx"][j, s],
                 sc["car_vy"][j, s]) for j in range(nc)]
        ego = (sc["ego_x"][s], sc["ego_y"][s], sc["ego_yaw_deg"][s], sc["ego_speed_mph"][s])
        prev = list(zip(sc["prev_x"][:npv, s], sc["prev_y"][:npv, s]))
        one = oracle_lib.one_scene(ego, prev, cars, int(sc["prev_target_lane"][s]))
        host = {k: v for k, v in one.items() if k != "struct"}
        ref = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], host, prm, info=True)
        srl.assert_effective(ref["info"], host, [], ladder=[0])
        ppamd.plan_reset(env["m"])
        nx, ny, tl = ppamd.plan_frame(env["m"], *ego, sc["prev_x"][:npv, s], sc["prev_y"][:npv, s], cars,
                                      target_lane=int(sc["prev_target_lane"][s]))
        n = int(ref["n_out"][0])
        assert len(nx) == n and tl == int(ref["info"]["target_lane"][0]), s
        assert np.isfinite(ref["next_x"][:n, 0]).all() and np.isfinite(nx).all(), s
        bound = srl.heading_bound(ref, srl.kept(host), meta["A"][s:s + 1])[0]
        e = max(np.abs(nx - ref["next_x"][:n, 0]).max(initial=0), np.abs(ny - ref["next_y"][:n, 0]).max(initial=0))
        assert e <= bound, (s, e, bound)
        a = srl.LADDER[meta["rung"][s]]
        worst[a] = max(worst.get(a, 0.0), float(e))
    ppamd.plan_reset(env["m"])
    print(f"pp_plan_frame: max |dxy| per rung (m): {srl.format_report(worst)}")


@pytest.mark.gpu
def test_large_map_all_paths(env):
    """A 2,000-waypoint map (read from global memory; no fused step) with ladder scenes, all paths."""
    import test_maps
    wx, wy = test_maps.loop_map(2000, seed=2000)
    m = ppamd.Map(wx, wy)
    sc, meta = srl.wound_heading_scenes(m, 600, seed=2000, first=2000)
    prm = ppamd.default_params(emit_paths=True)
    got = ev(env, to_dev(env, sc), prm, m=m)
    oracle_check(env, sc, meta, got, prm, what="2,000-waypoint map, all paths", wx=wx, wy=wy)
