"""Scene preparation (K1) at the sensor_fusion row counts the synthetic generator never makes.

The generator always reports 12 rows in 12 columns; the scene-preparation kernels branch on exactly
that number. These tests put every K1 variant on batches whose row count differs from lane to
lane, at every count 0 ... J of a J-column batch (J below, at and above the 16-key sorting
network, and more than two rounds of the widest group), against the oracle under the strict
contract, `pp_scene_info` included (oracle_lib.compare_info):

- the one-lane k_prep (3- and 4-wave builds): its 16-key Batcher network with pad keys, the
  identity order at 17 rows and with a negative id, equal float keys, a zero key;
- k_sort_cars (K0) ahead of it, for 2 <= J <= 16 columns;
- the grouped K1 at G = 2, 4, 8, 16: rounds of G rows, the rows loaded ahead (r < car_stride), the
  partial last round; and the K1 inside k_step_small and ahead of k_cand_small;
- n_cars > car_stride (clamped by every reader, as the oracle clamps it) and car_stride = 0 with
  empty and with null car arrays;
- the sorting rule's boundary at 15 and 16 Monte-Carlo draws.

The CPU test checks, with the oracle alone, that the scenes are worth running: every count occurs,
neighbouring lanes differ, and a K1 that dropped or added one row would change the outputs that are
compared."""
import math

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd

COLUMNS = [0, 1, 2, 3, 5, 8, 9, 12, 15, 16, 17, 18, 33]
S_ROWS = 1536                     # 24 waves: whole 256-lane blocks, every wave with mixed counts
CAR_FIELDS = ("car_x", "car_y", "car_vx", "car_vy")


def _ego_point(sc):
    """The point K1's distance keys are taken from: the last kept previous point when 10 are kept,
    the telemetry pose otherwise (k_sort_cars / prep_ego)."""
    kept = sc["n_prev"] >= ppamd.PREV_KEEP
    return np.where(kept, sc["prev_x"][9], sc["ego_x"]), np.where(kept, sc["prev_y"][9], sc["ego_y"])


def _d2(x, y, ex, ey):
    """The squared distance as the kernels form it (-ffp-contract=off: two products, one sum)."""
    dx, dy = x - ex, y - ey
    return dx * dx + dy * dy


def _key(d2):
    """The float sort key without its row nibble."""
    return np.float32(d2).view(np.uint32) & np.uint32(0xFFFFFFF0)


def count_step(M):
    """The smallest odd step >= 5 coprime to M (odd: coprime to a wave's 64 lanes)."""
    k = 5
    while math.gcd(k, M) != 1:
        k += 2
    return k


def row_counts(S, J, clamp=False):
    """n_cars per scene: a cycle through 0 ... J (0 ... J + 2 with `clamp`) with a step coprime to
    64 and to the cycle length, shifted by one per 64 scenes, so that the lanes of a wave differ
    and no count is tied to a residue of the scene index."""
    M = J + (3 if clamp else 1)
    s = np.arange(S, dtype=np.int64)
    return ((s * count_step(M) + s // 64) % M).astype(np.int32)


def row_edge_scenes(m, S, J, seed, clamp=False):
    """Host SoA scenes with car_stride = J for the row-count tests. Returns (scenes, notes); notes
    holds the indices of the scenes that carry each edge.

    - start: generator scenes; J > 12 puts generator batches side by side, J < 12 keeps the first
      J rows;
    - three scenes of four: every row is a car placed around the ego along its heading (-30 ...
      +35 m, lateral offsets of 4 m, speeds 0 ... 30 m/s along the heading), so the planner's
      result depends on which rows are counted; the others keep the generator's cars (rows beyond
      the generator's 12 are placed as well: another batch's cars are another ego's);
    - n_cars: row_counts (J + 1 and J + 2 only with `clamp`);
    - ids ascending and gappy; every 9th scene has one negative id (row 0: the identity order);
    - every 16th scene (s % 16 == 5), as far as its count allows: two counted cars at mirror-image
      positions about the key's ego point (equal squared distances), two whose squared distances
      differ by one double ulp (equal float keys: the row index decides), one exactly on the ego
      point (key 0);
    - s % 97 == 11: the ego 1,500 ... 4,000 m off the map (unmatched);
    - s % 97 == 50: a first frame (no previous path) with the ego at rest and row 0 a stopped car
      14.75 m ahead in its lane (LimitSpeed's KEEP window): counted, it holds the ego at speed 0,
      where the reference's step direction is 0/0 and the trajectory ends after one generated
      point (n_out < n_points). (An unmatched ego alone still gets all its points: the oracle
      gives n_out = n_points on every far-ego scene, and a standstill with kept points takes the
      fallback integrator, which fills the horizon.)"""
    rng = np.random.default_rng(seed)
    nb = max((J + 11) // 12, 1)
    bs = [ppamd.synth_host(m, S, seed=seed + i, first=0) for i in range(nb)]
    sc = {k: np.array(v, copy=True) for k, v in bs[0].items()}
    for k in CAR_FIELDS:
        sc[k] = np.ascontiguousarray(np.concatenate([b[k] for b in bs], 0)[:J])
    ids = np.cumsum(rng.integers(1, 9, (max(J, 1), S)), axis=0).astype(np.int32)[:J]
    neg = np.arange(S) % 9 == 4
    if J:
        ids[0, neg] = -1 - 3 * (np.arange(S)[neg] % 5)           # -1 (the sentinel), -4, ... -13
    sc["car_id"] = np.ascontiguousarray(ids)
    sc["n_cars"] = row_counts(S, J, clamp)
    live = np.minimum(sc["n_cars"], J)

    far = np.arange(S) % 97 == 11
    off = rng.uniform(1500, 4000, S)
    sc["prev_x"][:, far] += off[far]
    sc["ego_x"][far] += off[far]
    still = np.arange(S) % 97 == 50
    sc["n_prev"][still] = 0
    sc["ego_speed_mph"][still] = 0.0

    ex, ey = _ego_point(sc)
    ux, uy = sc["prev_x"][9] - sc["prev_x"][8], sc["prev_y"][9] - sc["prev_y"][8]
    nrm = np.hypot(ux, uy)
    yaw = np.deg2rad(sc["ego_yaw_deg"])
    ux = np.where(nrm > 1e-6, ux / np.maximum(nrm, 1e-12), np.cos(yaw))
    uy = np.where(nrm > 1e-6, uy / np.maximum(nrm, 1e-12), np.sin(yaw))
    nx, ny = uy, -ux                                             # +d direction

    def place(rows, mask, ds, lat, sp):
        for k, v in zip(CAR_FIELDS, (ex + ux * ds + nx * lat, ey + uy * ds + ny * lat, ux * sp, uy * sp)):
            sc[k][rows] = np.where(mask, v, sc[k][rows])

    placed = np.arange(S) % 4 != 3
    for j in range(J):
        ds = rng.uniform(-30, 35, S)
        lane = rng.choice([0, 0, -1, 1, -2, 2], S)               # lateral lanes about the ego's
        lat = 4.0 * lane + rng.uniform(-0.4, 0.4, S)
        sp = rng.uniform(0, 30, S)
        place(j, placed | still | (j >= 12), ds, lat, sp)
    if J:
        place(0, still, 14.75, 0.0, 0.0)

    notes = {"far": np.nonzero(far)[0], "still": np.nonzero(still & (live > 0))[0],
             "neg": np.nonzero(neg & (live > 0))[0], "mirror": [], "ulp": [], "zero": []}
    for s in np.nonzero(np.arange(S) % 16 == 5)[0]:
        c = int(live[s])
        free = list(range(c))
        pri = ["mirror", "ulp", "zero"]
        pri = pri[(s // 16) % 3:] + pri[:(s // 16) % 3]
        for kind in pri:
            if kind == "zero" and len(free) >= 1:
                j = free.pop(len(free) // 2)
                sc["car_x"][j, s], sc["car_y"][j, s] = ex[s], ey[s]
                notes["zero"].append(s)
            elif kind == "mirror" and len(free) >= 2:
                ja, jb = free.pop(0), free.pop(-1)
                for _ in range(64):
                    ds, lat = rng.uniform(6, 30), 4.0 * rng.integers(-1, 2) + rng.uniform(-0.4, 0.4)
                    # offsets on a 2^-20 m grid: ego + offset and ego - offset are exact
                    ox = np.round((ux[s] * ds + nx[s] * lat) * 2.0 ** 20) / 2.0 ** 20
                    oy = np.round((uy[s] * ds + ny[s] * lat) * 2.0 ** 20) / 2.0 ** 20
                    xa, ya, xb, yb = ex[s] + ox, ey[s] + oy, ex[s] - ox, ey[s] - oy
                    if xa - ex[s] == ox and xb - ex[s] == -ox and ya - ey[s] == oy and yb - ey[s] == -oy:
                        break
                else:
                    raise AssertionError("no exact mirror pair")
                sc["car_x"][ja, s], sc["car_y"][ja, s] = xa, ya
                sc["car_x"][jb, s], sc["car_y"][jb, s] = xb, yb
                notes["mirror"].append(s)
            elif kind == "ulp" and len(free) >= 2:
                ja, jb = free.pop(0), free.pop(0)
                xa, ya = sc["car_x"][ja, s], sc["car_y"][ja, s]
                if not placed[s] or far[s]:                      # a car near the ego to copy
                    xa, ya = ex[s] + ux[s] * 17.0 + nx[s] * 0.25, ey[s] + uy[s] * 17.0 + ny[s] * 0.25
                    sc["car_x"][ja, s], sc["car_y"][ja, s] = xa, ya
                xb, yb = _one_ulp_farther(xa, ya, ex[s], ey[s])
                sc["car_x"][jb, s], sc["car_y"][jb, s] = xb, yb
                sc["car_vx"][jb, s], sc["car_vy"][jb, s] = sc["car_vx"][ja, s], sc["car_vy"][ja, s]
                notes["ulp"].append(s)
    notes = {k: np.asarray(v, np.int64) for k, v in notes.items()}
    return sc, notes


def _one_ulp_farther(xa, ya, ex, ey):
    """A point within nanometres of (xa, ya) (some thousand coordinate ulps) whose squared distance to (ex, ey), as the
    kernels form it, is the next double after (xa, ya)'s. Moving k ulps in x and l in y changes
    the squared distance by about 2 dx ulp(x) k + 2 dy ulp(y) l; for each l the best k is taken
    and the candidates are checked exactly."""
    d0 = _d2(xa, ya, ex, ey)
    want = np.nextafter(d0, np.inf)
    hx, hy = np.spacing(abs(xa)), np.spacing(abs(ya))
    gx, gy = 2 * (xa - ex) * hx, 2 * (ya - ey) * hy
    if abs(gx) < abs(gy):                                        # solve for the coarser direction
        xb, yb = _one_ulp_farther(ya, xa, ey, ex)
        return yb, xb
    for l0 in range(0, 400000, 20000):
        l = np.concatenate([np.arange(l0, l0 + 20000), -np.arange(l0 + 1, l0 + 20001)]).astype(np.float64)
        k = np.round(((want - d0) - gy * l) / gx)
        xb, yb = xa + k * hx, ya + l * hy
        hit = np.nonzero(_d2(xb, yb, ex, ey) == want)[0]
        if hit.size:
            return float(xb[hit[0]]), float(yb[hit[0]])
    raise AssertionError("no point one ulp farther")


def lower_counts(sc):
    """The same scenes with one row fewer wherever there is one."""
    out = dict(sc)
    out["n_cars"] = np.where(sc["n_cars"] > 0, sc["n_cars"] - 1, 0).astype(np.int32)
    return out


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    return {"m": ppamd.Map(wx, wy), "wx": wx, "wy": wy, "olib": oracle_lib.load_oracle()}


_cache = {}


def scenes_and_oracle(env, J, S=S_ROWS, clamp=False):
    """row_edge_scenes(J) and the oracle's all-paths evaluation with info, once per module run
    (the reference every variant is compared with; never modified)."""
    key = (J, S, clamp)
    if key not in _cache:
        sc, notes = row_edge_scenes(env["m"], S, J, seed=9100 + J, clamp=clamp)
        prm = ppamd.default_params(emit_paths=True)
        ref = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, prm, info=True)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = (sc, notes, ref)
    return _cache[key]


@pytest.mark.parametrize("J", COLUMNS)
def test_row_edge_scenes_cover_the_branches(cpu, J):
    """Conditions on the inputs (oracle only): the scenes reach the branches, and the compared
    outputs depend on the last counted row. What the oracle gives (J: scenes with rows whose
    in_lane_car >= 0 / whose n_matched_cars changes with one row fewer / where a decision or cost
    changes; bounds 10 %, 90 %, 20 %): 1: 24/99/83 %, 2: 34/99/78, 3: 39/99/70, 5: 50/99/62,
    8: 62/98/52, 9: 64/99/48, 12: 69/99/44, 15: 74/99/41, 16: 76/99/38, 17: 78/99/39, 18: 80/99/37,
    33: 89/99/26; n_out < n_points in 4 to 13 scenes per J."""
    S = S_ROWS
    sc, notes, ref = scenes_and_oracle(cpu, J)
    n = sc["n_cars"]
    assert sc["car_id"].shape == (J, S) and all(sc[k].shape == (J, S) for k in CAR_FIELDS)
    assert n.min() == 0 and n.max() == J and np.unique(n).size == J + 1
    for b in range(0, S, 64):
        assert np.unique(n[b:b + 64]).size >= min(J + 1, 8), b
    for s in range(S):                                           # ascending ids over the counted rows
        assert (np.diff(sc["car_id"][:n[s], s]) > 0).all(), s
    for k in ("ego_x", "ego_y", "prev_x", "prev_y") + CAR_FIELDS:
        assert np.isfinite(sc[k]).all() and (np.abs(sc[k]) < 1e4).all(), k
    st = ref["status"].view(np.uint32)
    assert (st[notes["far"]] & ppamd.STATUS_BITS["EGO_UNMATCHED"]).sum() >= 4
    if J == 0:
        return
    short = np.nonzero(ref["n_out"] < 50)[0]                     # held at a standstill: fewer points
    assert short.size > 0 and np.isin(short, notes["still"]).all(), short
    info = ref["info"]
    has = n >= 1
    bits = ppamd.STATUS_BITS
    in_lane = float((info["in_lane_car"][has] >= 0).mean())
    assert in_lane >= 0.10, in_lane
    assert (st & bits["LANE_CLOSED"]).any()
    assert (st & (bits["BRAKE"] | bits["ADJUST"] | bits["KEEP"])).any()
    # the key edges are what they claim to be, as the kernels compute the keys
    ex, ey = _ego_point(sc)
    for kind in ("mirror", "ulp", "zero"):
        if J >= 2 or kind == "zero":
            assert notes[kind].size > 0, kind
    sorted_edges = 0
    for kind in ("mirror", "ulp", "zero"):
        for s in notes[kind]:
            d2 = _d2(sc["car_x"][:n[s], s], sc["car_y"][:n[s], s], ex[s], ey[s])
            if kind == "zero":
                assert (d2 == 0).any(), s
                continue
            srt = np.sort(d2)
            gap = srt[1:] == (srt[:-1] if kind == "mirror" else np.nextafter(srt[:-1], np.inf))
            assert gap.any(), (kind, s)
            i = int(np.nonzero(gap)[0][0])
            assert _key(srt[i]) == _key(srt[i + 1])
            sorted_edges += int(1 < n[s] <= 16 and (sc["car_id"][:n[s], s] >= 0).all())
    if 2 <= J:
        assert sorted_edges > 0                                  # some edge scene takes the network
    # sensitivity: one row fewer
    low = oracle_lib.oracle_eval(cpu["olib"], cpu["wx"], cpu["wy"], lower_counts(sc),
                                 ppamd.default_params(), info=True)
    dn = float((low["info"]["n_matched_cars"][has] != info["n_matched_cars"][has]).mean())
    diff = low["winner"] != ref["winner"]
    for k in ("target_lane", "in_lane_car", "lane_open_mask"):
        diff |= low["info"][k] != info[k]
    diff |= ~np.all((low["cost"] == ref["cost"]) | (np.isnan(low["cost"]) & np.isnan(ref["cost"])), axis=1)
    dd = float(diff[has].mean())
    print(f"J = {J}: in_lane_car >= 0 in {in_lane:.1%} of the scenes with rows; one row fewer changes "
          f"n_matched_cars in {dn:.1%} and a decision or cost in {dd:.1%}; n_out < 50 in "
          f"{int((ref['n_out'] < 50).sum())} scenes; edges mirror/ulp/zero "
          f"{notes['mirror'].size}/{notes['ulp'].size}/{notes['zero'].size}")
    assert dn >= 0.90, dn
    assert dd >= 0.20, dd


# ---- GPU ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    wx, wy = oracle_lib.highway_map()
    return {"torch": torch, "m": ppamd.Map(wx, wy), "wx": wx, "wy": wy,
            "olib": oracle_lib.load_oracle(), "dev": torch.device("cuda", 0)}


def to_dev(env, d):
    return {k: (None if v is None else env["torch"].from_numpy(np.ascontiguousarray(v)).to(env["dev"]))
            for k, v in d.items()}


def run_gpu(env, d, prm, info=True, group=0, waves=0, shape=ppamd.SHAPE_AUTO, k0=0):
    S = int(d["ego_x"].shape[0])
    r = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"], info=info)
    with ppamd.debug(ppamd.DBG_PREP_GROUP, group), ppamd.debug(ppamd.DBG_PREP_WAVES, waves), \
            ppamd.debug(ppamd.DBG_SHAPE, shape), ppamd.debug(ppamd.DBG_SORT_CARS, k0):
        ppamd.evaluate(env["m"], d, prm, r, device=0)
    env["torch"].cuda.synchronize()
    return ppamd.result_to_numpy(r)


def same_bits(a, b):
    if a.dtype.names:
        return all(same_bits(a[f], b[f]) for f in a.dtype.names if f != "_pad")
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def without_paths(ref):
    return {k: v for k, v in ref.items() if k not in ("paths", "path_len")}


# every K1 the library has, in reference mode without paths: (name, run_gpu settings)
K1_VARIANTS = [("k_prep w3", dict(group=1, waves=3, shape=ppamd.SHAPE_SPLIT)),
               ("k_prep w4", dict(group=1, waves=4, shape=ppamd.SHAPE_SPLIT)),
               ("K0 + k_prep w3", dict(group=1, waves=3, shape=ppamd.SHAPE_SPLIT, k0=1)),
               ("K0 + k_prep w4", dict(group=1, waves=4, shape=ppamd.SHAPE_SPLIT, k0=1)),
               ("grouped G=2", dict(group=2, shape=ppamd.SHAPE_SPLIT)),
               ("grouped G=4", dict(group=4, shape=ppamd.SHAPE_SPLIT)),
               ("grouped G=8", dict(group=8, shape=ppamd.SHAPE_SPLIT)),
               ("grouped G=16", dict(group=16, shape=ppamd.SHAPE_SPLIT)),
               ("k_cand_small", dict(shape=ppamd.SHAPE_CAND_SMALL)),
               ("k_step_small", dict(shape=ppamd.SHAPE_STEP))]


def check_every_k1(env, sc, ref, label, variants=K1_VARIANTS, paths=True):
    """Every variant against the oracle (compare + compare_info), and the paths-free results bit
    for bit against the first variant's. Every variant runs; a failure names all that failed."""
    ref0 = without_paths(ref)
    d = to_dev(env, sc)
    prm = ppamd.default_params()
    first = None
    worst, failed = {}, []
    runs = [(name, prm, kw) for name, kw in variants]
    if paths:
        runs.append(("k_prep w3 with paths", ppamd.default_params(emit_paths=True),
                     dict(group=1, waves=3, shape=ppamd.SHAPE_SPLIT)))
    for name, p, kw in runs:
        got = run_gpu(env, d, p, **kw)
        try:
            oracle_lib.compare(got, ref if p.emit_paths else ref0)
            for f, e in oracle_lib.compare_info(got["info"], ref["info"]).items():
                worst[f] = max(worst.get(f, 0.0), e)
        except AssertionError as exc:
            failed.append(f"{name}: {str(exc)[:300]}")
        if p.emit_paths:
            continue
        if first is None:
            first = got
        diff = [k for k, v in first.items() if not same_bits(got[k], v)]
        if diff:
            failed.append(f"{name}: not the bits of {runs[0][0]} in {diff}")
    print(f"{label}: info max |d| vs the oracle " + ", ".join(f"{f} {e:.3e}" for f, e in worst.items()))
    assert not failed, f"{label}: {len(failed)} failures: " + "; ".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("J", COLUMNS)
def test_row_counts_every_k1_vs_oracle(env, J):
    """Every count 0 ... J in a J-column batch, counts differing from lane to lane, through every
    K1 variant. K0 runs for 2 <= J <= 16 columns; elsewhere the switch must change nothing."""
    sc, _, ref = scenes_and_oracle(env, J)
    check_every_k1(env, sc, ref, f"J = {J}")
    if J == 0:
        # the same batch with null car pointers (car_stride = 0 needs none, include/pp.h / pp_eval)
        nul = dict(sc)
        for k in ("car_id",) + CAR_FIELDS:
            nul[k] = None
        assert ppamd.scene_struct(nul).car_stride == 0 and not ppamd.scene_struct(nul).car_x
        check_every_k1(env, nul, ref, "J = 0, null car arrays")


@pytest.mark.gpu
@pytest.mark.parametrize("J", [5, 16, 17])
@pytest.mark.parametrize("D", [15, 16])
def test_row_counts_draw_boundary(env, J, D):
    """The one-lane K1 sorts a scene's rows below kSortDmax = 16 draws and keeps the identity
    order from 16 on; batches this small would otherwise take the grouped K1. The Monte-Carlo
    contract of test_montecarlo.TestMonteCarloGPU.check (costs and draw-averaged costs within 1e-9,
    decisions, output counts and flags exact, the nominal trajectory within TOL), taken through
    oracle_lib.compare: the standstill scenes' nominal trajectory is the reference's 0/0 NaN point,
    which that check's plain maximum cannot hold against itself, and compare requires the NaN
    pattern to be identical (and the points beyond n_out to be 0)."""
    S = 256
    sc, _ = row_edge_scenes(env["m"], S, J, seed=9300 + J)
    prm = ppamd.default_params(n_speeds=1, cost_mode=ppamd.COST_COMFORT, n_draws=D)
    ref = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, prm, info=False)
    assert ref["cost"].shape == (S, D * ppamd.NUM_LANES)
    d = to_dev(env, sc)
    for k0 in ((0, 1) if D == 15 else (0,)):
        got = run_gpu(env, d, prm, info=False, group=1, k0=k0)
        oracle_lib.compare(got, ref)
        np.testing.assert_allclose(got["draw_mean_cost"], ref["draw_mean_cost"], rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("J", [3, 16])
def test_rows_beyond_columns_are_clamped(env, J):
    """n_cars = J + 1 and J + 2 in a J-column batch: k_sort_cars, k_prep and the grouped K1 clamp
    the count to car_stride before they read a row, as the oracle does, so the result is that of
    n_cars = J."""
    S = 512
    sc, _ = row_edge_scenes(env["m"], S, J, seed=9500 + J, clamp=True)
    assert (sc["n_cars"] == J + 1).any() and (sc["n_cars"] == J + 2).any()
    ref = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, ppamd.default_params(emit_paths=True),
                                 info=True)
    over = sc["n_cars"] > J
    assert (ref["info"]["n_matched_cars"][over] <= J).all()
    variants = [v for v in K1_VARIANTS if v[0] in ("k_prep w3", "K0 + k_prep w3", "grouped G=16")]
    check_every_k1(env, sc, ref, f"clamp, J = {J}", variants=variants, paths=False)
