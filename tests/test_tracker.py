"""The tracker between the sensor and the planner (pp_track_frame, pp_track_frame_host,
pp_rollout_tracked, pp_rollout_sweep_tracked; DESIGN.md "Tracker").

The oracle is an ordered restatement of csrc/pp_tracker.h's definitions in NumPy over all scenes of a
frame at once. The arithmetic is the header's operations in the header's order (NumPy fuses nothing), so
every value must be equal bit for bit; the merge is restated from sets instead of cursors: which rows are
accepted (a running maximum), which tracks they match (an id comparison of every row with every track),
and for a track without a row how many tracks and rows come before it. Ids, counts, src and misses are
exact. A second, textbook filter (4 states per car, F P F' + Q, np.linalg.solve) checks the arithmetic
itself, and a statistical test that the filter filters.

CPU: the host twin against the restatement (a hand-made car, seeded 12-frame sequences at the block
edges and with 100 cars, the identity tracker, row rules and the room rule, NaN and infinite rows, reset,
sharding, every argument error). GPU: device == host bits; the identity tracker against
pp_rollout_sensed; a real tracker frame by frame against the host twin and pp_eval; the tracker without a
sensor; the sweep against its calls made by hand."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import DT, Geo, many_car_traffic, move, random_frame, same_bits, to_np

NONE, NEW, UPDATED, COASTED = 0, 1, 2, 3
ROWS = ["car_id", "car_x", "car_y", "car_vx", "car_vy"]
SLOTS = ppamd.TRACK_SLOT_FIELDS                        # id, misses, x, y, vx, vy, ppp, ppv, pvv
SIZES = [1, 63, 64, 65, 257, 1000]
COASTS = [0, 2, 10]
FRAMES = 12
NAN, INF = float("nan"), float("inf")
SENSOR = dict(seed=77, first_scene=3, pos_sigma=0.4, pos_sigma_per_m=0.01, vel_sigma=0.3, dropout_prob=0.3,
              occlusion_radius=1.5)
MATCHED = dict(meas_pos_sigma=0.4, meas_pos_sigma_per_m=0.01, meas_vel_sigma=0.3, acc_sigma=1.0)


# ---- the ordered restatement ----------------------------------------------------------------------------
def fin(x):
    return x - x == 0


def oracle(z, cfg, consume, st):
    """One frame over the rows `z` (a scene dict) from the state `st`: the state afterwards. Everything a
    call does not write is copied from `st`."""
    K, S = z["car_id"].shape
    out = {k: v.copy() for k, v in st.items()}
    sx = np.arange(S)
    f = st["frame"].astype(np.int64)
    rb = f & 1
    wb = rb ^ 1
    n = np.clip(z["n_cars"], 0, K)
    nold = np.where(f == 0, 0, np.clip(st["n_tracks"][rb, sx], 0, K))
    kk = np.arange(K)[:, None]
    o = {k: st[k].reshape(2, K, S)[rb[None], kk, sx[None]] for k in SLOTS}          # the old bank [K, S]
    tvalid = kk < nold[None]
    dt = consume * 0.02
    d2, q = dt * dt, cfg.acc_sigma * cfg.acc_sigma
    q4, q3, q2 = (q * (d2 * d2)) / 4.0, (q * (d2 * dt)) / 2.0, q * d2
    rvv = cfg.meas_vel_sigma * cfg.meas_vel_sigma
    with np.errstate(all="ignore"):
        # predict, every old track
        p = {"x": o["x"] + dt * o["vx"], "y": o["y"] + dt * o["vy"], "vx": o["vx"], "vy": o["vy"],
             "ppp": (o["ppp"] + dt * ((2.0 * o["ppv"]) + (dt * o["pvv"]))) + q4,
             "ppv": (o["ppv"] + dt * o["pvv"]) + q3, "pvv": o["pvv"] + q2}
        # accepted rows: ascending ids
        rid = z["car_id"]
        acc = np.zeros((K, S), bool)
        last = np.full(S, -2 ** 62, np.int64)
        for r in range(K):
            acc[r] = (r < n) & (rid[r] > last)
            last = np.where(acc[r], rid[r], last)
        eq = acc[:, None] & tvalid[None] & (rid[:, None] == o["id"][None])           # [row, track, S]
        has, m = eq.any(1), eq.argmax(1)
        g = {k: np.take_along_axis(p[k], m, 0) for k in p}                          # the row's track, predicted
        zx, zy, zvx, zvy = z["car_x"], z["car_y"], z["car_vx"], z["car_vy"]
        ax, ay = zx - z["ego_x"], zy - z["ego_y"]
        if cfg.meas_pos_sigma != 0 or cfg.meas_pos_sigma_per_m != 0:
            sp = cfg.meas_pos_sigma + cfg.meas_pos_sigma_per_m * np.sqrt(ax * ax + ay * ay)
        else:
            sp = np.zeros((K, S))
        rpp = sp * sp
        spp, spv, svv = g["ppp"] + rpp, g["ppv"], g["pvv"] + rvv
        det = spp * svv - spv * spv
        ix, ivx, iy, ivy = zx - g["x"], zvx - g["vx"], zy - g["y"], zvy - g["vy"]
        kal = has & ~((rpp == 0) & (rvv == 0)) & (det > 0) & fin(det) & fin(ix) & fin(ivx) & fin(iy) & fin(ivy)
        k11, k12 = (g["ppp"] * svv - g["ppv"] * spv) / det, (g["ppv"] * spp - g["ppp"] * spv) / det
        k21, k22 = (g["ppv"] * svv - g["pvv"] * spv) / det, (g["pvv"] * spp - g["ppv"] * spv) / det
        row = {"id": rid, "misses": np.zeros((K, S), np.int32),
               "x": np.where(kal, g["x"] + (k11 * ix + k12 * ivx), zx),
               "vx": np.where(kal, g["vx"] + (k21 * ix + k22 * ivx), zvx),
               "y": np.where(kal, g["y"] + (k11 * iy + k12 * ivy), zy),
               "vy": np.where(kal, g["vy"] + (k21 * iy + k22 * ivy), zvy),
               "ppp": np.where(kal, g["ppp"] - (k11 * g["ppp"] + k12 * g["ppv"]), rpp),
               "ppv": np.where(kal, g["ppv"] - (k11 * g["ppv"] + k12 * g["pvv"]), 0.0),
               "pvv": np.where(kal, g["pvv"] - (k21 * g["ppv"] + k22 * g["pvv"]), rvv)}
    # tracks without a row: the rows before them, and the room rule in track order
    before = (acc[:, None] & (rid[:, None] < o["id"][None])).sum(0)                 # accepted rows before track t
    gt = acc[:, None] & (rid[:, None] > o["id"][None])
    consumed = np.where(gt.any(0), gt.argmax(0), n[None])                           # rows consumed on reaching it
    cand = tvalid & ~eq.any(0) & (o["misses"] < cfg.max_coast)
    kept, tpos = np.zeros((K, S), bool), np.zeros((K, S), np.int64)
    coasts = np.zeros(S, np.int64)
    for t in range(K):
        tpos[t] = before[t] + coasts
        kept[t] = cand[t] & (tpos[t] + (n - consumed[t]) < K)
        coasts += kept[t]
    rpos = np.cumsum(acc, 0) - 1 + (kept[None] & (o["id"][None] < rid[:, None])).sum(1)
    trk = dict(p, id=o["id"], misses=o["misses"] + 1)
    for src, pos, vals, code in ((acc, rpos, row, np.where(has, UPDATED, NEW)), (kept, tpos, trk, COASTED)):
        a, s = np.nonzero(src)
        w = pos[a, s]
        for k in SLOTS:
            out[k].reshape(2, K, S)[wb[s], w, s] = vals[k][a, s]
        for k, kk_ in zip(ROWS, ("id", "x", "y", "vx", "vy")):
            out[k][w, s] = vals[kk_][a, s]
        out["src"][w, s] = code[a, s] if isinstance(code, np.ndarray) else code
    count = acc.sum(0) + kept.sum(0)
    out["src"][kk >= count[None]] = NONE
    out["n_tracks"][wb, sx] = count
    out["n_cars"][:] = count
    out["frame"][:] = f + 1
    return out


# ---- inputs -----------------------------------------------------------------------------------------------
_ENV = {}


def env():
    if not _ENV:
        wx, wy = oracle_lib.highway_map()
        m = ppamd.Map(wx, wy)
        _ENV.update(m=m, geo=Geo(m.geometry()))
    return _ENV


def rows_of(geo, ex, ey, tr, counts=None, id_step=1):
    """The telemetry of a frame: the ego at (ex, ey) and the traffic's cars as rows (car j with id
    j id_step + id_step - 1), the first counts[s] of them in scene s."""
    J, S = int(tr["n_cars"]), len(ex)
    sc = ppamd.alloc_scenes(S, max(J, 1))
    sc["ego_x"][:], sc["ego_y"][:] = ex, ey
    p, u = geo.car(tr["lane"][:J], tr["seg"][:J], tr["t"][:J], tr["offset"][:J])
    sc["car_x"][:J], sc["car_y"][:J] = p[..., 0], p[..., 1]
    sc["car_vx"][:J], sc["car_vy"][:J] = u[..., 0] * tr["speed"][:J], u[..., 1] * tr["speed"][:J]
    sc["car_id"][:J] = (np.arange(J) * id_step + id_step - 1)[:, None]
    sc["n_cars"][:] = J if counts is None else counts
    return sc


_SEQ = {}


def sequence(S, seed=11):
    """FRAMES consecutive frames of S scenes as the tracker sees them: random_frame's cars (0 to 12 per
    scene, ids 2, 5, 8, ..; S = "big": 64 scenes of 100 cars) driving on at their speeds, 3 steps a frame,
    the ego 0.5 m a frame, through pp_sense_frame_host with noise, dropout 0.3 and occlusion (one
    sensor state carried). Made once per S and shared: nothing writes to it (the tests check that)."""
    if S not in _SEQ:
        e = env()
        geo = e["geo"]
        if S == "big":
            sc0, tr = many_car_traffic(e["m"], 64, 5, n=100)
            ex, ey, counts, step = sc0["ego_x"].copy(), sc0["ego_y"].copy(), None, 1
        else:
            fr = random_frame(geo, S, 12, seed + S)
            ex, ey, tr, step = fr["ex"], fr["ey"], fr["traffic"], 3
            counts = np.random.default_rng(seed).integers(0, 13, S)
        cfg = ppamd.default_sensor_cfg(**SENSOR)
        sensor = None
        frames = []
        for f in range(FRAMES):
            truth = rows_of(geo, ex + 0.5 * f, ey, tr, counts, step)
            sensor = sensor if sensor is not None else ppamd.alloc_sensor(len(ex), truth["car_id"].shape[0])
            ppamd.sense_frame(truth, sensor, cfg, host=True)
            frames.append(to_np(ppamd.sensed_scenes(truth, sensor)))
            move(geo, tr, 3)
        _SEQ[S] = frames
    return _SEQ[S]


def host_track(z, cfg, state=None, consume=3):
    st = state if state is not None else ppamd.alloc_tracker(len(z["ego_x"]), z["car_id"].shape[0])
    ppamd.track_frame(z, st, cfg, consume, host=True)
    return st


def one_scene(K, cars, ego=(0.0, 0.0)):
    """A scene of K rows holding `cars`: (id, x, y, vx, vy) each."""
    sc = ppamd.alloc_scenes(1, K)
    sc["ego_x"][0], sc["ego_y"][0] = ego
    sc["n_cars"][0] = len(cars)
    for r, c in enumerate(cars):
        for k, v in zip(ROWS, c):
            sc[k][r, 0] = v
    return sc


def rows_list(st, s=0):
    return [tuple(st[k][r, s] for k in ROWS) for r in range(st["n_cars"][s])]


# ---- CPU: the host twin against the restatement ---------------------------------------------------------------
def test_hand_made_car():
    """Reported noiselessly for 5 frames, then absent: coasts by x += dt vx for exactly max_coast frames
    and is gone in the next. Reported again after a coast it is UPDATED, after the deletion NEW."""
    K, coast, consume = 3, 4, 3
    dt = consume * 0.02
    cfg = ppamd.default_tracker_cfg(max_coast=coast, **MATCHED)
    st = ppamd.alloc_tracker(1, K)
    x, y, vx, vy = 10.0, -2.0, 20.0, 0.5
    for f in range(5):
        z = one_scene(K, [(7, x, y, vx, vy)])
        want = oracle(z, cfg, consume, st)
        host_track(z, cfg, st)
        same_bits(want, st, f"frame {f}")
        assert st["src"][:, 0].tolist() == [NEW if f == 0 else UPDATED, NONE, NONE]
        (j, tx, ty, tvx, tvy), = rows_list(st)
        assert j == 7 and abs(tx - x) < 1e-9 and abs(ty - y) < 1e-9 and abs(tvx - vx) < 1e-9 and abs(tvy - vy) < 1e-9
        x, y = x + dt * vx, y + dt * vy
    (_, cx, cy, cvx, cvy), = rows_list(st)
    gone = one_scene(K, [])
    for f in range(coast):
        want = oracle(gone, cfg, consume, st)
        host_track(gone, cfg, st)
        same_bits(want, st, f"coast {f}")
        cx, cy = cx + dt * cvx, cy + dt * cvy
        assert st["src"][:, 0].tolist() == [COASTED, NONE, NONE] and rows_list(st) == [(7, cx, cy, cvx, cvy)]
        assert st["misses"].reshape(2, K)[st["frame"][0] & 1, 0] == f + 1
        if f == 1:                                          # reported again during the coast
            u = to_np(st)
            host_track(one_scene(K, [(7, cx + dt * cvx + 1.0, cy + dt * cvy, cvx, cvy)]), cfg, u)
            assert u["src"][0, 0] == UPDATED and u["misses"].reshape(2, K)[u["frame"][0] & 1, 0] == 0
            assert cx + dt * cvx < u["car_x"][0, 0] < cx + dt * cvx + 1.0
    want = oracle(gone, cfg, consume, st)
    host_track(gone, cfg, st)
    same_bits(want, st, "deleted")
    assert st["n_cars"][0] == 0 and (st["src"] == NONE).all() and st["car_x"][0, 0] == cx
    host_track(one_scene(K, [(7, 3.0, 0.0, 1.0, 0.0)]), cfg, st)
    assert st["src"][:, 0].tolist() == [NEW, NONE, NONE] and rows_list(st) == [(7, 3.0, 0.0, 1.0, 0.0)]


def run_sequence(S, cfg, check=True):
    """The sequence of S through one carried state: the states after every frame (host twin), each
    compared with the restatement from the state before."""
    frames = sequence(S)
    st = ppamd.alloc_tracker(len(frames[0]["ego_x"]), frames[0]["car_id"].shape[0])
    states = []
    for f, z in enumerate(frames):
        want = oracle(z, cfg, 3, st) if check else None
        host_track(z, cfg, st)
        if check:
            same_bits(want, st, f"S={S} frame {f}")
        states.append(to_np(st))
    return states


def check_sequence(S):
    before = [to_np(z) for z in sequence(S)]
    seen, deleted = set(), 0
    for mc in COASTS:
        states = run_sequence(S, ppamd.default_tracker_cfg(max_coast=mc, **MATCHED))
        for f, st in enumerate(states):
            seen |= set(np.unique(st["src"]).tolist())
            ids = [set(st["car_id"][:st["n_cars"][s], s].tolist()) for s in range(0, len(st["n_cars"]), 7)]
            if f:
                deleted += sum(len(a - b) for a, b in zip(was, ids))
            was = ids
            used = np.arange(1, st["car_id"].shape[0])[:, None] < st["n_cars"][None]
            assert (np.diff(st["car_id"].astype(np.int64), axis=0) > 0)[used].all()         # ascending ids
            if mc == 0:
                assert (st["src"] != COASTED).all()
    for a, b in zip(before, sequence(S)):
        same_bits(a, b, "input")
    return seen, deleted


@pytest.mark.parametrize("S", SIZES)
def test_sequences_vs_restatement(S):
    seen, deleted = check_sequence(S)
    if S >= 63:
        assert seen == {NONE, NEW, UPDATED, COASTED} and deleted > 0


def test_hundred_car_sequence_vs_restatement():
    z = sequence("big")[0]
    assert z["car_id"].shape == (100, 64)
    seen, deleted = check_sequence("big")
    assert {NEW, UPDATED, COASTED} <= seen and deleted > 0


@pytest.mark.parametrize("S", SIZES + ["big"])
def test_identity_tracker(S):
    """The default configuration: the tracked rows are the input rows bit for bit, nothing coasts."""
    st = ppamd.alloc_tracker(len(sequence(S)[0]["ego_x"]), sequence(S)[0]["car_id"].shape[0])
    for f, z in enumerate(sequence(S)):
        prev = to_np(st)
        host_track(z, ppamd.default_tracker_cfg(), st)
        live = np.arange(z["car_id"].shape[0])[:, None] < z["n_cars"][None]
        want = {k: np.where(live, z[k], prev[k]) for k in ROWS}
        want["n_cars"] = z["n_cars"]
        same_bits(want, {k: st[k] for k in want}, f"identity frame {f}")
        assert np.isin(st["src"][live], (NEW, UPDATED)).all() and (st["src"][~live] == NONE).all()
        if f == 0:
            assert (st["src"][live] == NEW).all()
        assert (st["frame"] == f + 1).all()


def test_row_rules_and_room_rule():
    cfg = ppamd.default_tracker_cfg(max_coast=5, **MATCHED)
    # a non-ascending or duplicate id is skipped; a negative count is none, a count beyond K is K
    z = one_scene(6, [(5, 1.0, 0, 0, 0), (3, 2.0, 0, 0, 0), (5, 3.0, 0, 0, 0), (8, 4.0, 0, 0, 0), (8, 5.0, 0, 0, 0),
                      (-2, 6.0, 0, 0, 0)])
    st = host_track(z, cfg)
    same_bits(oracle(z, cfg, 3, ppamd.alloc_tracker(1, 6)), st, "skips")
    assert [(r[0], r[1]) for r in rows_list(st)] == [(5, 1.0), (8, 4.0)] and st["src"][:, 0].tolist() == [NEW, NEW, 0, 0, 0, 0]
    z["n_cars"][0] = -4
    assert host_track(z, cfg)["n_cars"][0] == 0
    z["n_cars"][0] = 99
    assert host_track(z, cfg)["n_cars"][0] == 2
    # the room rule at K = 4, ids that change every frame: reported rows always fit, the coasting tracks
    # with the lowest ids fill what room is left
    K = 4
    st = ppamd.alloc_tracker(1, K)
    frames = [[10, 11, 12, 13], [20, 21, 22], [1, 30], [2, 3, 4, 40], []]
    wants = [[10, 11, 12, 13], [10, 20, 21, 22], [1, 10, 20, 30], [2, 3, 4, 40], [2, 3, 4, 40]]
    srcs = [[NEW] * 4, [COASTED, NEW, NEW, NEW], [NEW, COASTED, COASTED, NEW], [NEW] * 4, [COASTED] * 4]
    for ids, want, src in zip(frames, wants, srcs):
        z = one_scene(K, [(j, float(j), 0.0, 1.0, 0.0) for j in ids])
        o = oracle(z, cfg, 3, st)
        host_track(z, cfg, st)
        same_bits(o, st, f"room {ids}")
        assert st["car_id"][:st["n_cars"][0], 0].tolist() == want and st["src"][:len(src), 0].tolist() == src


def test_nan_and_infinite_rows_are_taken_outright():
    cfg = ppamd.default_tracker_cfg(max_coast=3, **MATCHED)
    K = 4
    st = ppamd.alloc_tracker(1, K)
    seqs = [[(1, 5.0, 1.0, 2.0, 0.0), (2, 9.0, 1.0, 2.0, 0.0), (3, 1.0, 2.0, 3.0, 4.0)],
            [(1, NAN, 1.0, 2.0, 0.0), (2, 9.1, INF, 2.0, 0.0), (3, 1.2, 2.2, -INF, 4.0)],
            [(1, 5.2, 1.0, 2.0, 0.0), (2, 9.2, 1.0, 2.0, 0.0), (3, 1.4, 2.4, 3.0, 4.0)],
            [(1, 5.3, 1.0, 2.0, 0.0), (2, 9.3, 1.0, 2.0, 0.0), (3, 1.6, 2.6, 3.0, 4.0)]]
    for f, cars in enumerate(seqs):
        z = one_scene(K, cars, ego=(0.5, 0.5))
        o = oracle(z, cfg, 3, st)
        host_track(z, cfg, st)
        same_bits(o, st, f"frame {f}")
        if f in (1, 2):                                     # the bad row, and the row after a bad state
            assert [tuple(np.asarray(r, float).tobytes() for r in rows_list(st))] == \
                   [tuple(np.asarray(c, float).tobytes() for c in cars)], f
    assert st["src"][:3, 0].tolist() == [UPDATED] * 3 and np.isfinite([r[1:] for r in rows_list(st)]).all()
    assert rows_list(st)[0][1] != 5.3                       # filtering again
    # a row at infinity from the ego with a range-dependent sigma: R is not finite, taken outright
    far = one_scene(K, [(1, 5.4, 1.0, 2.0, 0.0)], ego=(INF, 0.0))
    o = oracle(far, cfg, 3, st)
    host_track(far, cfg, st)
    same_bits(o, st, "ego at infinity")
    assert rows_list(st)[0] == (1, 5.4, 1.0, 2.0, 0.0)


def test_reset_by_zeroing_frame_alone():
    S = 65
    cfg = ppamd.default_tracker_cfg(max_coast=2, **MATCHED)
    z = sequence(S)[0]
    clean = host_track(z, cfg)
    dirty = run_sequence(S, cfg, check=False)[-1]
    before = to_np(dirty)
    dirty["frame"][:] = 0
    host_track(z, cfg, dirty)
    live = np.arange(12)[:, None] < clean["n_cars"][None]
    for k in ROWS + ["src"]:
        want = clean[k] if k == "src" else np.where(live, clean[k], before[k])     # rows beyond the count: left alone
        assert want.tobytes() == dirty[k].tobytes(), k
    bank = lambda st, k: np.where(live, st[k].reshape(2, 12, S)[1], 0)
    for k in SLOTS:
        assert bank(clean, k).tobytes() == bank(dirty, k).tobytes(), k
        assert before[k].reshape(2, 12, S)[0].tobytes() == dirty[k].reshape(2, 12, S)[0].tobytes()    # only read
    assert (dirty["frame"] == 1).all() and np.array_equal(dirty["n_tracks"][1], clean["n_tracks"][1])
    assert (before["n_cars"] != clean["n_cars"]).any()


def test_sharding():
    S = 1000
    cfg = ppamd.default_tracker_cfg(max_coast=2, **MATCHED)
    whole = run_sequence(S, cfg, check=False)[-1]
    for a, b in ((0, 500), (500, 1000)):
        st = ppamd.alloc_tracker(b - a, 12)
        for z in sequence(S):
            host_track({k: np.ascontiguousarray(v[..., a:b]) for k, v in z.items()}, cfg, st)
        same_bits({k: v[..., a:b] for k, v in whole.items()}, st, f"shard {a}")


def test_argument_errors():
    S, R = 6, 4
    sc = ppamd.alloc_scenes(S, R)
    sc["n_cars"][:] = 3
    st = ppamd.alloc_tracker(S, R)
    for v in st.values():
        v[...] = 77
    ref = C.byref

    def call(sc_=sc, cfg=None, st_=st, device=None, consume=3, **over):
        b = ppamd.scene_struct(sc_) if sc_ is not None else None
        for k, v in over.items():
            setattr(b, k, v)
        c = cfg if cfg is not None else ppamd.default_tracker_cfg()
        X = ppamd.tracker_struct(st_) if st_ is not None else None
        args = (ref(b) if b is not None else None, ref(c) if c != "null" else None, consume,
                ref(X) if X is not None else None)
        if device is None:
            return ppamd.lib.pp_track_frame_host(*args)
        return ppamd.lib.pp_track_frame(*args, device, None)

    bad_cfgs = [dict(meas_pos_sigma=-1.0), dict(meas_pos_sigma=NAN), dict(meas_pos_sigma=INF),
                dict(meas_pos_sigma_per_m=-0.1), dict(meas_pos_sigma_per_m=INF), dict(meas_pos_sigma_per_m=NAN),
                dict(meas_vel_sigma=-2.0), dict(meas_vel_sigma=NAN), dict(meas_vel_sigma=INF), dict(acc_sigma=-1.0),
                dict(acc_sigma=INF), dict(acc_sigma=NAN), dict(max_coast=-1)]
    for device in (None, 0):
        assert call(sc_=None, device=device) == -1 and call(cfg="null", device=device) == -1
        assert call(st_=None, device=device) == -1
        for k in ("ego_x", "ego_y", "n_cars", "car_id", "car_x", "car_y", "car_vx", "car_vy"):
            assert call(device=device, **{k: None}) == -1, k
        for k in st:
            assert call(st_=dict(st, **{k: None}), device=device) == -1, k
        for kw in bad_cfgs:
            assert call(cfg=ppamd.default_tracker_cfg(**kw), device=device) == -1, kw
        assert call(device=device, n_scenes=-1) == -1 and call(device=device, car_stride=-1) == -1
        assert call(device=device, car_stride=ppamd.MAX_CARS + 1) == -1
        assert call(device=device, consume=0) == -1 and call(device=device, consume=-3) == -1
    assert call(device=-1) == -1 and call(device=99) == -1
    assert all((v == 77).all() for v in st.values())
    # the limits themselves are fine; no scenes: nothing is written
    assert call(n_scenes=0, consume=1) == 0 and call(device=0, n_scenes=0) == 0
    assert all((v == 77).all() for v in st.values())
    d = ppamd.default_tracker_cfg()
    assert (d.meas_pos_sigma, d.meas_pos_sigma_per_m, d.meas_vel_sigma, d.acc_sigma, d.max_coast) == (0, 0, 0, 0, 0)


def test_rollout_and_sweep_argument_errors():
    """A lone tracker configuration or state, a tracker the stage would refuse (the second of two sets), no
    tracker sets: PP_ERR_ARG before anything is launched (host arrays stand in for the device buffers:
    nothing may touch them)."""
    m = env()["m"]
    S, n = 8, 12
    good = ppamd.default_params()
    sc = ppamd.add_car_table(ppamd.alloc_scenes(S, n), slots=n)
    tr, res = ppamd.alloc_traffic(S, n), ppamd.alloc_result(S, good)
    tr["n_cars"] = n
    jd, fo, lc = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n), ppamd.alloc_lane_change(S, n)
    st, se, tk = ppamd.alloc_judge_stats(4, 8), ppamd.alloc_sensor(S, n), ppamd.alloc_tracker(S, n)
    bufs = (sc, tr, res, jd, fo, lc, st, se, tk)
    before = [to_np(d) for d in bufs]
    ref = C.byref
    b, T, R = ppamd.scene_struct(sc), ppamd.traffic_struct(tr), ppamd.result_struct(res)
    J, F, L, O = ppamd.judge_struct(jd), ppamd.follow_struct(fo), ppamd.lane_change_struct(lc), ppamd.stats_struct(st)
    X, Y = ppamd.sensor_struct(se), ppamd.tracker_struct(tk)
    oks, okt = ppamd.default_sensor_cfg(), ppamd.default_tracker_cfg()

    def rollout(tcfg, tstate, sensor=True):
        rc = ppamd.RolloutCfg(2, 3, 300.0)
        return ppamd.lib.pp_rollout_tracked(m.handle, ref(b), ref(T), ref(good), ref(rc), ref(R), None, 0, None,
                                            ref(ppamd.default_judge_cfg()), ref(J), ref(ppamd.default_follow_cfg()),
                                            ref(F), ref(ppamd.default_lane_change_cfg()), ref(L),
                                            ref(oks) if sensor else None, ref(X) if sensor else None, tcfg, tstate)

    for sensor in (True, False):
        assert rollout(ref(okt), None, sensor) == -1 and rollout(None, ref(Y), sensor) == -1
        assert rollout(ref(ppamd.default_tracker_cfg(acc_sigma=-1.0)), ref(Y), sensor) == -1
        assert rollout(ref(ppamd.default_tracker_cfg(max_coast=-1)), ref(Y), sensor) == -1
        assert rollout(ref(okt), ref(ppamd.tracker_struct(dict(tk, src=None))), sensor) == -1
        assert rollout(ref(okt), ref(ppamd.tracker_struct(dict(tk, ppv=None))), sensor) == -1

    def sweep(trackers, tstate=True, sensors=True, sstate=True, sets=None):
        P = len(trackers or [okt])
        sets = sets or [good] * P
        arr = (ppamd.Params * len(sets))(*sets)
        sarr = (ppamd.SensorCfg * P)(*[oks] * P) if sensors else None
        tarr = (ppamd.TrackerCfg * P)(*trackers) if trackers else None
        cfg = ppamd.SweepCfg(len(sets), 0, 1, 0, ppamd.RolloutCfg(2, 3, 300.0), ppamd.SummaryCfg(4, 8, 0, 100.0, 0, 0))
        return ppamd.lib.pp_rollout_sweep_tracked(
            m.handle, arr, ref(cfg), ref(ppamd.default_episode_cfg()), ref(ppamd.default_judge_cfg()),
            ref(ppamd.default_follow_cfg()), ref(ppamd.default_lane_change_cfg()), ref(b), ref(T), ref(R), ref(J),
            ref(F), ref(L), ref(O), 0, None, sarr, ref(X) if sstate else None, tarr, ref(Y) if tstate else None)

    assert sweep(None) == -1 and sweep([okt], tstate=False) == -1
    assert sweep([okt], sensors=False) == -1 and sweep([okt], sstate=False) == -1
    assert sweep([okt, ppamd.default_tracker_cfg(meas_pos_sigma=-1.0)]) == -1
    assert sweep([okt, ppamd.default_tracker_cfg(max_coast=-2)]) == -1
    assert sweep([okt, okt], sets=[good, ppamd.default_params(n_speeds=9)]) == -1
    for d, was in zip(bufs, before):
        same_bits(was, to_np(d), "buffers")


# ---- CPU: two independent checks of the arithmetic --------------------------------------------------------------
# The largest relative difference |a - b| / max(|b|, 1) between the matrix-form filter and the ordered
# restatement (both test-side) over the sequences of 65 and 257 scenes with max_coast 2, states and
# covariances: measured 1.305e-15 at 65 scenes (1,939 updates) and 8.758e-16 at 257 (6,882 updates), a
# few units in the last place. Other seeds are allowed 16 times the larger.
MATRIX_MEASURED = 1.305e-15


def matrix_filter(frames, cfg, consume, states):
    """One textbook 4-state filter per car ([x, vx, y, vy], F P F' + Q, gain by np.linalg.solve),
    started, updated, coasted and deleted as `states` (the tracker's, per frame) say. Returns the largest
    relative difference of its states and covariances to the tracker's."""
    dt = consume * DT
    F2 = np.array([[1.0, dt], [0.0, 1.0]])
    F = np.kron(np.eye(2), F2)
    q = cfg.acc_sigma ** 2
    Q = np.kron(np.eye(2), q * np.array([[dt ** 4 / 4, dt ** 3 / 2], [dt ** 3 / 2, dt ** 2]]))
    worst, n_upd = 0.0, 0
    S = len(frames[0]["ego_x"])
    filt = [dict() for _ in range(S)]
    for z, st in zip(frames, states):
        b = int(st["frame"][0] & 1)
        bank = {k: st[k].reshape(2, -1, S)[b] for k in SLOTS}
        for s in range(S):
            rows = {int(z["car_id"][r, s]): r for r in range(z["n_cars"][s])}
            nxt = {}
            for o in range(st["n_cars"][s]):
                j, src = int(st["car_id"][o, s]), st["src"][o, s]
                if src != COASTED:
                    r = rows[j]
                    zz = np.array([z["car_x"][r, s], z["car_vx"][r, s], z["car_y"][r, s], z["car_vy"][r, s]])
                    rho = np.hypot(zz[0] - z["ego_x"][s], zz[2] - z["ego_y"][s])
                    rpp = (cfg.meas_pos_sigma + cfg.meas_pos_sigma_per_m * rho) ** 2
                    R = np.diag([rpp, cfg.meas_vel_sigma ** 2] * 2)
                if src == NEW:
                    x, P = zz, R
                else:
                    x, P = filt[s][j]
                    x, P = F @ x, F @ P @ F.T + Q
                    if src == UPDATED:
                        G = np.linalg.solve((P + R).T, P.T).T                   # P (P + R)^-1
                        x, P = x + G @ (zz - x), P - G @ P
                        n_upd += 1
                nxt[j] = (x, P)
                got = np.array([bank[k][o, s] for k in ("x", "vx", "y", "vy", "ppp", "ppv", "pvv")])
                ref = np.array([x[0], x[1], x[2], x[3], P[0, 0], P[0, 1], P[1, 1]])
                worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))))
                assert abs(P[2, 2] - P[0, 0]) <= 1e-12 * P[0, 0] and abs(P[0, 2]) + abs(P[1, 3]) < 1e-12   # one 2x2
            filt[s] = nxt
    return worst, n_upd


@pytest.mark.parametrize("S", [65, 257])
def test_textbook_matrix_filter(S):
    cfg = ppamd.default_tracker_cfg(max_coast=2, **MATCHED)
    states = run_sequence(S, cfg, check=False)
    worst, n_upd = matrix_filter(sequence(S), cfg, 3, states)
    print(f"matrix form against the host twin, S={S}: {n_upd} updates, largest relative difference {worst:.3e}")
    assert n_upd > 20 * S
    assert worst <= 16 * MATRIX_MEASURED, worst


def test_the_filter_filters():
    """12,000 constant-velocity cars (1000 scenes x 12), sensed with pos_sigma 0.5 and vel_sigma 0.5, no
    dropout; the matched filter with acc_sigma 0. At the 20th frame the tracked positions' mean squared
    error must be below half the raw reports'. (Averaging 20 positions alone leaves sigma^2 / 20; the
    sample variance of 24,000 errors has a relative standard deviation near 1 %.)"""
    S, K, consume, sig = 1000, 12, 3, 0.5
    rng = np.random.default_rng(5)
    x0, y0 = rng.uniform(-200, 200, (K, S)), rng.uniform(-10, 10, (K, S))
    vx, vy = rng.uniform(0, 25, (K, S)), rng.uniform(-1, 1, (K, S))
    scfg = ppamd.default_sensor_cfg(seed=9, pos_sigma=sig, vel_sigma=sig)
    tcfg = ppamd.default_tracker_cfg(meas_pos_sigma=sig, meas_vel_sigma=sig)
    sensor, st = ppamd.alloc_sensor(S, K), ppamd.alloc_tracker(S, K)
    truth = ppamd.alloc_scenes(S, K)
    truth["n_cars"][:] = K
    truth["car_id"][:] = np.arange(K)[:, None]
    truth["car_vx"][:], truth["car_vy"][:] = vx, vy
    for f in range(20):
        t = f * consume * DT
        truth["car_x"][:], truth["car_y"][:] = x0 + vx * t, y0 + vy * t
        ppamd.sense_frame(truth, sensor, scfg, host=True)
        host_track(ppamd.sensed_scenes(truth, sensor), tcfg, st, consume)
    assert (st["n_cars"] == K).all() and (st["src"] == UPDATED).all()
    mse = lambda d: float(np.mean((d["car_x"] - truth["car_x"]) ** 2 + (d["car_y"] - truth["car_y"]) ** 2) / 2)
    raw, tracked = mse(sensor), mse(st)
    print(f"mean squared position error at frame 20: raw {raw:.5f} m^2, tracked {tracked:.5f} m^2")
    assert abs(raw - sig * sig) < 0.05 * sig * sig
    assert tracked < 0.5 * raw


# ---- GPU ------------------------------------------------------------------------------------------------------
NOISY = dict(seed=123, pos_sigma=0.5, pos_sigma_per_m=0.01, vel_sigma=0.5, dropout_prob=0.2, occlusion_radius=1.5)
NOISY_MATCHED = dict(meas_pos_sigma=0.5, meas_pos_sigma_per_m=0.01, meas_vel_sigma=0.5, acc_sigma=1.0)
TABLE = ppamd.TABLE_FIELDS_I + ppamd.TABLE_FIELDS_F


@pytest.mark.gpu
class TestTrackerGPU:
    @pytest.fixture(scope="class")
    def genv(self):
        import torch
        e = env()
        return {"m": e["m"], "geo": e["geo"], "torch": torch, "dev": torch.device("cuda", 0)}

    def upload(self, genv, d):
        t = genv["torch"]
        return {k: (t.from_numpy(v).to(genv["dev"]) if isinstance(v, np.ndarray) else v) for k, v in d.items()}

    def device_check(self, genv, S):
        frames = sequence(S)
        n, R = len(frames[0]["ego_x"]), frames[0]["car_id"].shape[0]
        up = [self.upload(genv, z) for z in frames]
        for mc in COASTS:
            cfg = ppamd.default_tracker_cfg(max_coast=mc, **MATCHED)
            sd = ppamd.alloc_tracker(n, R, xp="torch", device=genv["dev"])
            sh = ppamd.alloc_tracker(n, R)
            for f, (z, zd) in enumerate(zip(frames, up)):    # a fresh state, then carried
                ppamd.track_frame(zd, sd, cfg, 3, device=0)
                host_track(z, cfg, sh)
                genv["torch"].cuda.synchronize()
                same_bits(sh, ppamd.tracker_to_numpy(sd), f"S={S} max_coast={mc} frame {f}")
        for z, zd in zip(frames, up):
            same_bits(z, to_np(zd), "input")

    @pytest.mark.parametrize("S", SIZES)
    def test_device_equals_host_bits(self, genv, S):
        self.device_check(genv, S)

    def test_device_equals_host_bits_hundred_cars(self, genv):
        self.device_check(genv, "big")

    def start(self, genv, S, seed=31):
        dev, m = genv["dev"], genv["m"]
        st = {"judge": ppamd.alloc_judge(S, xp="torch", device=dev),
              "follow": ppamd.alloc_follow(S, 12, xp="torch", device=dev),
              "lane_change": ppamd.alloc_lane_change(S, 12, xp="torch", device=dev),
              "sensor": ppamd.alloc_sensor(S, 12, xp="torch", device=dev),
              "tracker": ppamd.alloc_tracker(S, 12, xp="torch", device=dev)}
        st["scenes"], st["traffic"] = ppamd.synth_episode(m, S, seed=seed, device=0, judge=st["judge"],
                                                          follow=st["follow"])
        st["result"] = ppamd.alloc_result(S, ppamd.default_params(), xp="torch", device=dev)
        return st

    def drive(self, genv, st, F, scfg=None, tcfg=None, tracked=True, sensor=True, log=None, sensor_range=300.0):
        prm = ppamd.default_params()
        if tracked:
            ppamd.rollout_tracked(genv["m"], st["scenes"], st["traffic"], prm, st["result"], st["follow"],
                                  st["lane_change"], st["sensor"] if sensor else None, st["tracker"], F, 3,
                                  sensor_range, judge=st["judge"], scfg=scfg, tcfg=tcfg, log=log)
        else:
            ppamd.rollout_sensed(genv["m"], st["scenes"], st["traffic"], prm, st["result"], st["follow"],
                                 st["lane_change"], st["sensor"], F, 3, sensor_range, judge=st["judge"], scfg=scfg,
                                 log=log)
        genv["torch"].cuda.synchronize()

    WORLD = ["scenes", "traffic", "result", "judge", "follow", "lane_change", "sensor"]

    def same_world(self, a, b, what, keys=None):
        for k in keys or self.WORLD:
            same_bits(to_np(a[k]), to_np(b[k]), f"{what} {k}")

    def test_identity_tracker_drives_as_sensed(self, genv):
        S, F = 1000, 40
        scfg = ppamd.default_sensor_cfg(**NOISY)
        plain, ident = self.start(genv, S), self.start(genv, S)
        self.drive(genv, plain, F, scfg, tracked=False)
        self.drive(genv, ident, F, scfg)
        self.same_world(plain, ident, "identity")
        tk, se = ppamd.tracker_to_numpy(ident["tracker"]), ppamd.sensor_to_numpy(ident["sensor"])
        assert (tk["frame"] == F).all() and (to_np(plain["judge"])["dist"] > 1).any()
        assert np.isin(tk["src"], (NONE, NEW, UPDATED)).all() and (tk["src"] == UPDATED).any()
        live = np.arange(12)[:, None] < se["n_cars"][None]
        same_bits({k: np.where(live, se[k], 0) for k in ROWS}, {k: np.where(live, tk[k], 0) for k in ROWS}, "rows")

    def test_real_tracker_frame_by_frame(self, genv):
        """20 one-frame calls of a matched tracker (max_coast 5) behind a noisy sensor over 300 scenes: each
        frame's tracked rows are the host twins' on the telemetry the frame began with, pp_eval on that
        telemetry with those rows gives the logged winner and plan and the frame's car table; one 20-frame
        call ends in the same bits; the drive is not the identity tracker's."""
        S, F, t, m = 300, 20, genv["torch"], genv["m"]
        scfg = ppamd.default_sensor_cfg(**NOISY)
        tcfg = ppamd.default_tracker_cfg(max_coast=5, **NOISY_MATCHED)
        prm = ppamd.default_params()
        step, once, ident = self.start(genv, S), self.start(genv, S), self.start(genv, S)
        hs, ht = ppamd.alloc_sensor(S, 12), ppamd.alloc_tracker(S, 12)
        srcs = set()
        for f in range(F):
            snap = {k: v.clone() for k, v in step["scenes"].items()}
            log = ppamd.alloc_log(1, S, prm.n_points, xp="torch", device=genv["dev"])
            self.drive(genv, step, 1, scfg, tcfg, log=log)
            truth = to_np(snap)
            ppamd.sense_frame(truth, hs, scfg, host=True)
            host_track(ppamd.sensed_scenes(truth, hs), tcfg, ht)
            tk = ppamd.tracker_to_numpy(step["tracker"])
            same_bits(hs, ppamd.sensor_to_numpy(step["sensor"]), f"frame {f} sensed")
            same_bits(ht, tk, f"frame {f} tracked")
            srcs |= set(np.unique(tk["src"]).tolist())
            res = ppamd.alloc_result(S, prm, xp="torch", device=genv["dev"])
            ppamd.evaluate(m, ppamd.tracked_scenes(snap, step["tracker"]), prm, res, device=0)
            t.cuda.synchronize()
            got, lg = ppamd.result_to_numpy(res), to_np(log)
            same_bits({"winner": lg["winner"][0], "n_out": lg["n_out"][0], "x": lg["plan_x"][0], "y": lg["plan_y"][0]},
                      {"winner": got["winner"], "n_out": got["n_out"], "x": got["next_x"], "y": got["next_y"]},
                      f"frame {f} plan")
            same_bits({k: to_np(snap)[k] for k in TABLE}, {k: to_np(step["scenes"])[k] for k in TABLE},
                      f"frame {f} table")
            assert np.array_equal(lg["n_cars"][0], truth["n_cars"])               # the log's count: the truth's
        assert srcs == {NONE, NEW, UPDATED, COASTED}
        self.drive(genv, once, F, scfg, tcfg)
        self.same_world(step, once, "20 x 1 == 1 x 20", self.WORLD + ["tracker"])
        self.drive(genv, ident, F, scfg)
        a, b = to_np(ident["scenes"]), to_np(once["scenes"])
        assert not np.array_equal(a["ego_x"], b["ego_x"]) or not np.array_equal(a["ego_y"], b["ego_y"])

    def test_tracker_without_a_sensor_coasts_cars_leaving_the_range(self, genv):
        """No sensor, sensor_range 60 m, max_coast 50: the tracker reads the truth rows. A car that leaves the
        range stays in the planner's rows as COASTED and its car-table entry goes on moving, where the
        identity tracker leaves the entry of a car that is not reported as it was."""
        S, F, t, m = 300, 20, genv["torch"], genv["m"]
        prm = ppamd.default_params()
        coasted = moved = frozen = unreported = 0
        for tcfg, ident in ((ppamd.default_tracker_cfg(max_coast=50), False), (ppamd.default_tracker_cfg(), True)):
            st = self.start(genv, S)
            ht = ppamd.alloc_tracker(S, 12)
            had = None
            for f in range(F):
                snap = {k: v.clone() for k, v in st["scenes"].items()}
                self.drive(genv, st, 1, tcfg=tcfg, sensor=False, sensor_range=60.0)
                truth, after = to_np(snap), to_np(st["scenes"])
                host_track(truth, tcfg, ht)
                tk = ppamd.tracker_to_numpy(st["tracker"])
                same_bits(ht, tk, f"frame {f} tracked")
                res = ppamd.alloc_result(S, prm, xp="torch", device=genv["dev"])
                ppamd.evaluate(m, ppamd.tracked_scenes(snap, st["tracker"]), prm, res, device=0)
                t.cuda.synchronize()
                same_bits({k: to_np(snap)[k] for k in TABLE}, {k: after[k] for k in TABLE}, f"frame {f} table")
                had = had if had is not None else [set()] * S
                for s in range(S):
                    rows = set(truth["car_id"][:truth["n_cars"][s], s].tolist())
                    got = dict(zip(tk["car_id"][:tk["n_cars"][s], s].tolist(), tk["src"][:tk["n_cars"][s], s].tolist()))
                    for j in had[s] - rows:                 # in the planner's rows last frame, out of range now
                        if ident:
                            assert j not in got
                            unreported += 1
                            frozen += all(truth[k][j, s] == after[k][j, s] for k in ("tab_s", "tab_d", "tab_valid"))
                        else:
                            assert got[j] == COASTED, (f, s, j)
                            coasted += 1
                            moved += bool(after["tab_valid"][j, s]) and truth["tab_s"][j, s] != after["tab_s"][j, s]
                    had[s] = set(got)
            assert (ppamd.sensor_to_numpy(st["sensor"])["frame"] == 0).all()      # the sensor never ran
        assert coasted > 50 and moved > 0.5 * coasted, (coasted, moved)
        assert unreported > 20 and frozen == unreported, (unreported, frozen)

    def test_sweep_equals_the_calls_made_by_hand(self, genv):
        """Three sets (identity; matched; matched with max_coast 10) behind one noisy sensor, 1,024 scenes in
        G = 2 groups, 30 frames."""
        S, E, F, B, hm, G = 1024, 512, 30, 64, 64.0, 2
        m, t = genv["m"], genv["torch"]
        scfg = ppamd.default_sensor_cfg(**dict(NOISY, pos_sigma=1.0, dropout_prob=0.3))
        matched = dict(NOISY_MATCHED, meas_pos_sigma=1.0)
        trackers = [ppamd.default_tracker_cfg(), ppamd.default_tracker_cfg(**matched),
                    ppamd.default_tracker_cfg(max_coast=10, **matched)]
        sets = [ppamd.default_params()] * 3
        stats, buf = ppamd.rollout_sweep(m, sets, S, F, scenes_per_group=E, seed=31, hist_bins=B, hist_max=hm,
                                         sensors=[scfg] * 3, trackers=trackers)
        plain, _ = ppamd.rollout_sweep(m, sets[:1], S, F, scenes_per_group=E, seed=31, hist_bins=B, hist_max=hm,
                                       sensors=[scfg])
        t.cuda.synchronize()
        stats, plain = to_np(stats), to_np(plain)
        assert (ppamd.tracker_to_numpy(buf["tracker"])["frame"] == F).all()
        assert (ppamd.sensor_to_numpy(buf["sensor"])["frame"] == F).all()
        rows = lambda p: {k: v[..., p * G:(p + 1) * G] for k, v in stats.items()}
        for p, tcfg in enumerate(trackers):
            st = self.start(genv, S)
            self.drive(genv, st, F, scfg, tcfg)
            hand = ppamd.judge_summary(st["judge"], S, E, hist_bins=B, hist_max=hm, m=m, device=0)
            t.cuda.synchronize()
            same_bits(to_np(hand), rows(p), f"set {p}")
        same_bits(plain, rows(0), "identity set == pp_rollout_sweep_sensed")
        for p in (1, 2):
            differ = [k for k in ("dist_sum", "clean_dist_sum", "min_sep") if not np.array_equal(rows(0)[k], rows(p)[k])]
            assert differ, f"set {p} drove exactly as the identity tracker: the tracker did not reach the planner"
