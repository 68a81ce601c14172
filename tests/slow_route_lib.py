"""Scenes for the checked K2 route (k_prep's kLimSlow flag -> k_cand<true>, k_winner<true>,
k_winner_st<true>), and the comparison that goes with them (TEST INFRASTRUCTURE ONLY).

Two kinds of scene are flagged:
  - speed-edge scenes (speed_edge_scenes): a telemetry speed, a car speed or a ramp time outside
    the range proven for k_cand<false>'s unchecked reciprocals (csrc/pp_device.h speed_in_range);
  - wound-up headings (wound_heading_scenes): a start heading beyond kSlowAngle = 1e5 rad
    (csrc/pp_k_frame.h), as a simulator that never wraps its yaw would send it.

A telemetry speed or yaw is read only where the start pose reads it (csrc/pp_k_prep.h start_pose):
assert_effective checks that from the oracle's scene info, so an edge value written into a scene
that never reads it fails on the CPU.
"""
from __future__ import annotations

import numpy as np

import oracle_lib
from oracle_lib import ppamd


def speed_edge_scenes(m, S, seed=909, first=31337):
    """test_gpu_parity.py::test_speed_range_edges_vs_oracle's scenes: two of three are frame-0 scenes
    whose telemetry speed is -0, subnormal, tiny, huge or negative, and every other scene has a car
    just ahead whose velocity is 0, -0, subnormal or tiny, so k_prep flags kLimSlow scenes all
    through the batch and flagged groups interleave with fast ones."""
    sc = ppamd.synth_host(m, S, seed=seed, first=first)
    speeds = [-0.0, 0.0, 5e-324, 1e-310, 1e-300, 1e-40, 1e-18, 2.237e-17, 1e-12, 1e-6, 0.3,
              49.66, 3e6, 1e300, -3.0, -1e-300, 2.237 * 22.2]
    vels = [0.0, -0.0, 5e-324, 1e-300, 1e-25, 1e-9, 3.0]
    p9x, p9y = sc["prev_x"][9], sc["prev_y"][9]
    hx, hy = p9x - sc["prev_x"][8], p9y - sc["prev_y"][8]
    nrm = np.maximum(np.hypot(hx, hy), 1e-12)
    for s in range(S):
        if s % 3 != 2:
            sc["n_prev"][s] = 0
            sc["ego_speed_mph"][s] = speeds[s % len(speeds)]
        if s % 2 == 0:
            sc["car_x"][0, s] = p9x[s] + hx[s] / nrm[s] * 20.0
            sc["car_y"][0, s] = p9y[s] + hy[s] / nrm[s] * 20.0
            v = vels[(s // 2) % len(vels)]
            sc["car_vx"][0, s] = v
            sc["car_vy"][0, s] = v
    return sc


# |A| in rad: the control below kSlowAngle, just above it, either side of ppm::kMediumMax
# (823549.6), through the restated glibc reduction's range (up to 1e8 rad) and beyond it
LADDER = (9.4e4, 1.01e5, 8.2e5, 8.3e5, 6.3e6, 1.6e7, 9.4e7, 1.01e8, 6.3e8, 6.3e10)
K_SLOW_ANGLE = 1.0e5
WAY_NONE, WAY_FRAME0, WAY_STANDING = 0, 1, 2
LADDER_PERIOD = 3 * 2 * len(LADDER)       # scenes after which every (rung, sign, way) has occurred

# telemetry speeds and car velocities outside speed_in_range's [2^-60, 2^20] (or -0), with values
# inside it between them
EDGE_SPEEDS = (-0.0, 5e-324, 1e-300, 1e-18, 0.3, 3e6, 1e300, -3.0, 1e-40, 49.66)
EDGE_CAR_VELS = (1e-25, 1e-40, 0.0, 1e-100, 1e-30, 1e-9)


def wound_heading_scenes(m, S, seed=20240, first=4000):
    """Synthetic scenes of which two in three read the telemetry yaw, by the two ways start_pose has:
    scene s with s % 3 == 0 is a frame-0 scene (n_prev = 0; telemetry speed kept within 0..49 mph),
    s % 3 == 1 a scene whose last kept step stands still (prev[9] = prev[8]); s % 3 == 2 stays as
    generated, so flagged and fast scenes share groups. The yaw is the road heading (of the scene's
    own last previous step) plus 360 k degrees, the car still pointing along the road; k runs over
    LADDER (rung (s // 3) % 10) in both signs ((s // 30) % 2), so every (rung, sign, way) occurs
    once in LADDER_PERIOD = 60 scenes.

    Returns (scenes, meta): meta["rung"] [S] (index into LADDER, -1: ordinary), meta["way"] [S]
    (WAY_*), meta["A"] [S] (the start heading yaw * pi / 180 in rad, signed; 0 for ordinary scenes)."""
    sc = ppamd.synth_host(m, S, seed=seed, first=first)
    rung = np.full(S, -1, np.int32)
    way = np.zeros(S, np.int32)
    A = np.zeros(S)
    hx = sc["prev_x"][9] - sc["prev_x"][8]
    hy = sc["prev_y"][9] - sc["prev_y"][8]
    road_deg = np.degrees(np.arctan2(hy, hx))
    for s in range(S):
        j, q = s % 3, s // 3
        if j == 2:
            continue
        rung[s] = q % len(LADDER)
        sign = 1.0 if (q // len(LADDER)) % 2 == 0 else -1.0
        turns = np.rint(sign * LADDER[rung[s]] / (2 * np.pi))
        sc["ego_yaw_deg"][s] = road_deg[s] + 360.0 * turns
        A[s] = sc["ego_yaw_deg"][s] * np.pi / 180
        if j == 0:
            way[s] = WAY_FRAME0
            sc["n_prev"][s] = 0
            sc["ego_speed_mph"][s] = min(max(sc["ego_speed_mph"][s], 0.0), 49.0)
        else:
            way[s] = WAY_STANDING
            sc["n_prev"][s] = 10
            sc["prev_x"][9, s] = sc["prev_x"][8, s]
            sc["prev_y"][9, s] = sc["prev_y"][8, s]
    return sc, {"rung": rung, "way": way, "A": A}


def mixed_slow_scenes(m, S, seed=20241, first=5000):
    """wound_heading_scenes with speed-edge scenes among its ordinary third (scene s = 3 t + 2):
    t % 3 == 0 becomes a frame-0 scene with an EDGE_SPEEDS telemetry speed, t % 3 == 1 gets a car
    20 m ahead whose velocity is one of EDGE_CAR_VELS (a LimitSpeed target of that size), t % 3 == 2
    stays ordinary. meta gains "edge" (indices of the telemetry-speed scenes) and "car" (indices of
    the car scenes)."""
    sc, meta = wound_heading_scenes(m, S, seed, first)
    p9x, p9y = sc["prev_x"][9], sc["prev_y"][9]
    hx, hy = p9x - sc["prev_x"][8], p9y - sc["prev_y"][8]
    nrm = np.maximum(np.hypot(hx, hy), 1e-12)
    edge, car = [], []
    for s in range(2, S, 3):
        t = s // 3
        if t % 3 == 0:
            sc["n_prev"][s] = 0
            sc["ego_speed_mph"][s] = EDGE_SPEEDS[(t // 3) % len(EDGE_SPEEDS)]
            edge.append(s)
        elif t % 3 == 1:
            sc["car_x"][0, s] = p9x[s] + hx[s] / nrm[s] * 20.0
            sc["car_y"][0, s] = p9y[s] + hy[s] / nrm[s] * 20.0
            v = EDGE_CAR_VELS[(t // 3) % len(EDGE_CAR_VELS)]
            sc["car_vx"][0, s] = v
            sc["car_vy"][0, s] = v
            car.append(s)
    meta["edge"] = np.array(edge, np.int64)
    meta["car"] = np.array(car, np.int64)
    return sc, meta


def ladder_idx(meta):
    return np.nonzero(meta["rung"] >= 0)[0]


def assert_ladder_complete(meta, sub=None):
    """Every rung occurs in both signs and by both ways of reading the yaw (among scenes `sub`)."""
    sub = np.arange(len(meta["rung"])) if sub is None else np.asarray(sub)
    seen = {(int(meta["rung"][s]), bool(meta["A"][s] > 0), int(meta["way"][s])) for s in sub if meta["rung"][s] >= 0}
    want = {(r, sg, w) for r in range(len(LADDER)) for sg in (False, True) for w in (WAY_FRAME0, WAY_STANDING)}
    assert seen == want, f"ladder incomplete: {sorted(want - seen)} missing"
    for s in sub:
        r = meta["rung"][s]
        if r >= 0:        # the rung's magnitude, on the side of kSlowAngle and kMediumMax it was chosen for
            assert abs(abs(meta["A"][s]) / LADDER[r] - 1) < 2e-4, (s, meta["A"][s], LADDER[r])
    return len(seen)


def take(sc, sub):
    """Scenes `sub` of a host batch as a batch of their own (scenes are independent)."""
    return {k: np.ascontiguousarray(v[..., sub]) for k, v in sc.items()}


def take_result(r, sub):
    return {k: (np.ascontiguousarray(v[:, sub]) if k in ("next_x", "next_y") else v[sub]) for k, v in r.items()}


def kept(sc):
    """K per scene: the previous points kept (oracle/pp_oracle.c prep_scene: 10 or 0)."""
    return np.where(sc["n_prev"] >= ppamd.PREV_KEEP, ppamd.PREV_KEEP, 0).astype(np.int64)


def _polyline(x, y, lo, hi):
    """Arc length of points lo..hi-1 of (x, y) [N]; 0 where a point is not finite."""
    if hi - lo < 2:
        return 0.0
    d = np.hypot(np.diff(x[lo:hi]), np.diff(y[lo:hi]))
    return float(d[np.isfinite(d)].sum())


def heading_bound(ref, K, A):
    """Per-scene bound [S] on |dxy| between the library and the oracle for scenes with start heading
    A [S] (rad; 0: an ordinary scene, which keeps oracle_lib.TOL).

    The library turns the output frame by rotating (cos, sin) of the heading (frame_turn); the
    reference adds each turn to a double of magnitude |A| (tangle += rot, oracle/pp_oracle.c:891)
    and so loses up to ulp(|A|) / 2 of heading per adjusted step. A turn rotates the frame about the
    current output point, so a heading error d made at generated point i moves a later point j by
    d |p_j - p_i| <= d L, L the arc length of the generated points. With at most n adjusted steps
    the two sides differ by up to 0.5 ulp(|A|) n L, on top of TOL. n = n_out - K and L come from the
    ORACLE's output; with all paths n is the longest path_len - K and L the scene's longest
    candidate."""
    A = np.abs(np.asarray(A, np.float64))
    S = A.shape[0]
    K = np.asarray(K)
    n = (ref["n_out"] - K).astype(np.float64)
    L = np.zeros(S)
    for s in np.nonzero(A > 0)[0]:
        L[s] = _polyline(ref["next_x"][:, s], ref["next_y"][:, s], int(K[s]), int(ref["n_out"][s]))
        if "paths" in ref:
            n[s] = max(n[s], float(ref["path_len"][s].max() - K[s]))
            for c in range(ref["path_len"].shape[1]):
                p = ref["paths"][s, :, c]
                L[s] = max(L[s], _polyline(p[:, 0], p[:, 1], int(K[s]), int(ref["path_len"][s, c])))
    term = np.where(A > 0, 0.5 * np.spacing(A) * np.maximum(n, 0) * L, 0.0)
    return oracle_lib.TOL + term


def _scene_err(a, b, what):
    """Largest |a - b| per scene (axis 0) over the finite values; the NaN patterns identical and
    infinite values equal on both sides (oracle_lib.max_err's contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), f"{what}: NaN pattern differs at {np.count_nonzero(na != nb)} values"
    ia, ib = np.isinf(a), np.isinf(b)
    assert (ia == ib).all() and (a[ia] == b[ia]).all(), f"{what}: infinite values differ"
    fin = ~(na | ia)
    with np.errstate(invalid="ignore"):
        d = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)), 0.0)
    return d.reshape(d.shape[0], -1).max(axis=1) if d.size else np.zeros(d.shape[0])


def compare_bounded(got, ref, bound, check_cost=True):
    """oracle_lib.compare with a per-scene bound [S] on next_x/next_y/paths in place of TOL;
    everything else is compare's contract as it stands: winners, n_out, path_len and status exact,
    NaN patterns identical, points beyond n_out exactly 0, costs within 1e-9. Returns the per-scene
    largest |dxy| [S] (formed before the bound is asserted)."""
    S = got["winner"].shape[0]
    err = np.zeros(S)
    if "paths" in ref:
        assert (got["path_len"] == ref["path_len"]).all(), \
            f"path_len differs for {int((got['path_len'] != ref['path_len']).sum())} candidates"
        err = np.maximum(err, _scene_err(got["paths"], ref["paths"], "paths"))
    assert (got["winner"] == ref["winner"]).all(), \
        f"winner differs in {int((got['winner'] != ref['winner']).sum())} scenes"
    assert (got["n_out"] == ref["n_out"]).all()
    N = got["next_x"].shape[0]
    live = np.arange(N)[:, None] < got["n_out"][None, :]
    for k in ("next_x", "next_y"):
        pad = got[k][~live]
        assert (pad == 0).all(), f"{k}: {int(np.count_nonzero(~(pad == 0)))} points beyond n_out are not 0"
        err = np.maximum(err, _scene_err(np.where(live, got[k], 0.0).T, np.where(live, ref[k], 0.0).T, k))
    over = np.nonzero(~(err <= bound))[0]
    assert over.size == 0, (f"{over.size} scenes beyond their bound; first {int(over[0])}: "
                            f"{err[over[0]]:.3e} m > {bound[over[0]]:.3e} m")
    if check_cost:
        np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=1e-9)
    assert (got["status"] == ref["status"].view(np.uint32)).all(), \
        f"status differs in {int((got['status'] != ref['status'].view(np.uint32)).sum())} scenes"
    return err


def compare_mc_bounded(got, ref, bound):
    """tests/test_montecarlo.py TestMonteCarloGPU.check with the per-scene bound on the nominal
    trajectory: costs and draw means within 1e-9, decisions, output counts and flags exact."""
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=1e-9)
    assert (got["winner"] == ref["winner"]).all()
    np.testing.assert_allclose(got["draw_mean_cost"], ref["draw_mean_cost"], rtol=1e-9, atol=1e-9)
    assert (got["n_out"] == ref["n_out"]).all()
    N = got["next_x"].shape[0]
    live = np.arange(N)[:, None] < ref["n_out"][None, :]
    err = np.zeros(got["winner"].shape[0])
    for k in ("next_x", "next_y"):
        err = np.maximum(err, _scene_err(np.where(live, got[k], 0.0).T, np.where(live, ref[k], 0.0).T, k))
    over = np.nonzero(~(err <= bound))[0]
    assert over.size == 0, (f"{over.size} scenes beyond their bound; first {int(over[0])}: "
                            f"{err[over[0]]:.3e} m > {bound[over[0]]:.3e} m")
    assert (got["status"] == ref["status"].view(np.uint32)).all()
    return err


def rung_report(err, meta, sub=None, bound=None):
    """Largest |dxy| per rung over scenes `sub` (err is indexed like sub): {rung |A|: metres}, with
    the ordinary scenes under key 0.0; printed by every GPU case."""
    sub = np.arange(len(meta["rung"])) if sub is None else np.asarray(sub)
    rung = meta["rung"][sub]
    out = {}
    for r in range(-1, len(LADDER)):
        sel = rung == r
        if sel.any():
            out[0.0 if r < 0 else LADDER[r]] = float(err[sel].max())
    return out


def format_report(rep):
    return ", ".join(f"{'ordinary' if a == 0 else format(a, 'g')}: {e:.2e}" for a, e in rep.items())


def assert_effective(ref_info, sc, idx, ladder=None):
    """The inputs meant to reach the checked route are read at all. From the oracle's scene info
    (ref_info: INFO_DTYPE [S], of the same batch as sc):
      - every intended speed-edge scene `idx` takes its ego speed from the telemetry:
        info.ego_speed == ego_speed_mph / 2.237, bit for bit (a scene with kept previous points
        takes it from its last step instead, and the telemetry value is inert);
      - every ladder scene `ladder` reads the telemetry yaw: its pose is the telemetry pose (no
        previous points kept), or the last kept step stands still (prev[8] == prev[9], the pose at
        that point and the speed 0)."""
    idx = np.asarray(idx, np.int64)
    want = sc["ego_speed_mph"][idx] / 2.237
    have = np.ascontiguousarray(ref_info["ego_speed"][idx])
    inert = idx[want.view(np.uint64) != have.view(np.uint64)]
    assert inert.size == 0, (f"{inert.size} of {idx.size} speed-edge scenes do not read the telemetry speed "
                             f"(n_prev = {sc['n_prev'][inert[:8]].tolist()} ...): first {inert[:8].tolist()}")
    if ladder is None:
        return
    bad = []
    for s in np.asarray(ladder, np.int64):
        if sc["n_prev"][s] < ppamd.PREV_KEEP:
            ok = ref_info["ego_x"][s] == sc["ego_x"][s] and ref_info["ego_y"][s] == sc["ego_y"][s]
        else:
            ok = (sc["prev_x"][8, s] == sc["prev_x"][9, s] and sc["prev_y"][8, s] == sc["prev_y"][9, s]
                  and ref_info["ego_x"][s] == sc["prev_x"][9, s] and ref_info["ego_y"][s] == sc["prev_y"][9, s]
                  and ref_info["ego_speed"][s] == 0)
        if not ok:
            bad.append(int(s))
    assert not bad, f"{len(bad)} ladder scenes do not read the telemetry yaw: first {bad[:8]}"
