"""The sensor model between the world and the planner (pp_sense_frame, pp_sense_frame_host,
pp_rollout_sensed, pp_rollout_sweep_sensed; DESIGN.md "Sensor model").

The oracle is an independent restatement of the definitions in NumPy, over all scenes of a frame at
once: Philox4x32-10 and the Irwin-Hall unit written out here (and checked first against the library's
pp_sensor_gauss / pp_sensor_word), occlusion as a [row, row, scene] mask, the compaction as a running
count. It evaluates the same IEEE operations in the same order (NumPy fuses nothing), so fates, counts
and ids must be exact and every value equal bit for bit.

CPU: the host twin against the oracle (a hand-made scene, the identity sensor, seeded random frames at
the block edges and with 100 cars, keying, sharding, frames, a car at the ego's position, every
argument error, the draws' statistics). GPU: device == host bits; the identity sensor against
pp_rollout_lane_changing; a noisy drive frame by frame against the host twin and pp_eval; the truth
behind a noisy drive; the sweep against its calls made by hand."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import Geo, many_car_traffic, random_frame, same_bits, to_np

M32 = 0xFFFFFFFF
TAG = 0x53454E53
CAR_STRIDE = 256                   # PP_NOISE_CAR_STRIDE
NONE, REPORTED, OCCLUDED, DROPPED = 0, 1, 2, 3
ROWS = ["car_id", "car_x", "car_y", "car_vx", "car_vy"]
SIZES = [1, 63, 64, 65, 257, 1000]
NAN, INF = float("nan"), float("inf")


# ---- the oracle -------------------------------------------------------------------------------------
def philox4x32(seed, c0, c1, c2, c3):
    """Philox4x32-10 over arrays of counters (Salmon et al. 2011): four uint64 arrays of 32-bit words."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    c = [np.asarray(x, np.uint64) & np.uint64(M32) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    lo, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def ih_unit(c):
    """Irwin-Hall of the block's four uniforms (w + 0.5) 2^-32, to unit variance."""
    s = (c[0].astype(np.float64) + 0.5) * 2.0 ** -32
    for w in c[1:]:
        s = s + (w.astype(np.float64) + 0.5) * 2.0 ** -32
    return (s - 2.0) * 1.7320508075688772


def block(seed, gs, frame, car, q):
    gs = np.asarray(gs, np.int64).astype(np.uint64)
    b = ((np.asarray(frame, np.int64) * CAR_STRIDE + (np.asarray(car, np.int64) & M32)) * 8 + q) & M32
    return philox4x32(seed, gs & np.uint64(M32), gs >> np.uint64(32), b, TAG)


def oracle(sc, cfg, frame):
    """One frame over the truth `sc` (a scene dict) at carried frame numbers `frame` [S]: the state a
    zero-filled sensor state becomes (rows at and beyond n_cars stay 0)."""
    R, S = sc["car_id"].shape
    n = np.clip(sc["n_cars"], 0, R)
    live = np.arange(R)[:, None] < n[None]
    ax, ay = sc["car_x"] - sc["ego_x"], sc["car_y"] - sc["ego_y"]
    aa = ax * ax + ay * ay
    hidden = np.zeros((R, S), bool)
    if cfg.occlusion_radius > 0 and R:
        with np.errstate(all="ignore"):
            A = lambda v: v[:, None, :]                                  # the row r
            B = lambda v: v[None, :, :]                                  # the other row k
            u = (A(ax) * B(ax) + A(ay) * B(ay)) / A(aa)
            u = np.where(u < 0, 0.0, np.where(u > 1, 1.0, u))
            dx, dy = B(ax) - u * A(ax), B(ay) - u * A(ay)
            hit = (B(aa) < A(aa)) & (dx * dx + dy * dy <= cfg.occlusion_radius * cfg.occlusion_radius)
        hit &= B(live) & ~np.eye(R, dtype=bool)[:, :, None]
        hidden = hit.any(1) & live
    gs = cfg.first_scene + np.arange(S)
    w = block(cfg.seed, gs[None], frame[None], sc["car_id"], 4)[0]
    dropped = live & ~hidden & (w.astype(np.float64) * 2.0 ** -32 < cfg.dropout_prob)
    rep = live & ~hidden & ~dropped
    g = [ih_unit(block(cfg.seed, gs[None], frame[None], sc["car_id"], q)) for q in range(4)]
    sp = cfg.pos_sigma + cfg.pos_sigma_per_m * np.sqrt(aa)
    if cfg.pos_sigma == 0 and cfg.pos_sigma_per_m == 0:
        sp = np.zeros_like(aa)                   # exactly 0 whatever rho (a row at infinity included)
    val = {"car_id": sc["car_id"],
           "car_x": np.where(sp != 0, sc["car_x"] + sp * g[0], sc["car_x"]),
           "car_y": np.where(sp != 0, sc["car_y"] + sp * g[1], sc["car_y"]),
           "car_vx": sc["car_vx"] + cfg.vel_sigma * g[2] if cfg.vel_sigma != 0 else sc["car_vx"],
           "car_vy": sc["car_vy"] + cfg.vel_sigma * g[3] if cfg.vel_sigma != 0 else sc["car_vy"]}
    out = ppamd.alloc_sensor(S, R)
    rank = np.cumsum(rep, 0) - 1
    rr, ss = np.nonzero(rep)
    for k in ROWS:
        out[k][rank[rr, ss], ss] = val[k][rr, ss]
    out["n_cars"][:] = rep.sum(0)
    out["fate"][:] = np.where(live, np.where(hidden, OCCLUDED, np.where(dropped, DROPPED, REPORTED)), NONE)
    out["frame"][:] = frame + 1
    return out


def used_rows(st):
    """A state with the rows at and beyond n_cars (which a call does not write) zeroed."""
    out = {k: v.copy() for k, v in st.items()}
    dead = np.arange(st["car_id"].shape[0])[:, None] >= st["n_cars"][None]
    for k in ROWS:
        out[k][dead] = 0
    return out


# ---- inputs -------------------------------------------------------------------------------------------
_ENV = {}


def env():
    if not _ENV:
        wx, wy = oracle_lib.highway_map()
        m = ppamd.Map(wx, wy)
        _ENV.update(m=m, geo=Geo(m.geometry()))
    return _ENV


def truth_of(geo, ex, ey, tr, counts=None, id_step=1, R=None):
    """The telemetry of a frame: the ego at (ex, ey) and the traffic's cars as rows (car j with id
    j id_step + id_step - 1, so ids are not row numbers), the first counts[s] of them in scene s."""
    J, S = int(tr["n_cars"]), len(ex)
    sc = ppamd.alloc_scenes(S, R if R is not None else max(J, 1))
    sc["ego_x"][:], sc["ego_y"][:] = ex, ey
    if J:
        p, u = geo.car(tr["lane"][:J], tr["seg"][:J], tr["t"][:J], tr["offset"][:J])
        sc["car_x"][:J], sc["car_y"][:J] = p[..., 0], p[..., 1]
        sc["car_vx"][:J], sc["car_vy"][:J] = u[..., 0] * tr["speed"][:J], u[..., 1] * tr["speed"][:J]
        sc["car_id"][:J] = (np.arange(J) * id_step + id_step - 1)[:, None]
    sc["n_cars"][:] = J if counts is None else counts
    return sc


_FRAMES = {}


def random_truth(S, seed=11):
    """random_frame's cars as telemetry rows, 0 to 12 per scene, ids 2, 5, 8, ..; made once per S and
    shared: nothing writes to it (the tests check that)."""
    if (S, seed) not in _FRAMES:
        geo = env()["geo"]
        fr = random_frame(geo, S, 12, seed + S)
        counts = np.random.default_rng(seed).integers(0, 13, S)
        _FRAMES[S, seed] = truth_of(geo, fr["ex"], fr["ey"], fr["traffic"], counts, id_step=3)
    return _FRAMES[S, seed]


def hundred_car_truth():
    """64 scenes of 100 cars: every row of car_stride in use."""
    if "big" not in _FRAMES:
        e = env()
        sc, big = many_car_traffic(e["m"], 64, 5, n=100)
        _FRAMES["big"] = truth_of(e["geo"], sc["ego_x"], sc["ego_y"], big)
    return _FRAMES["big"]


def host_sense(sc, cfg, state=None):
    st = state if state is not None else ppamd.alloc_sensor(len(sc["ego_x"]), sc["car_id"].shape[0])
    ppamd.sense_frame(sc, st, cfg, host=True)
    return st


CFGS = [dict(occlusion_radius=r, dropout_prob=p, pos_sigma=0.4, pos_sigma_per_m=0.01, vel_sigma=0.3, seed=77,
             first_scene=3) for r in (0.0, 1.5) for p in (0.0, 0.3, 1.0)]


# ---- CPU ------------------------------------------------------------------------------------------------
def test_draws_are_the_stated_philox_blocks():
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
        scene = int(rng.integers(0, 2 ** 40))
        frame, car = int(rng.integers(0, 2 ** 31)), int(rng.integers(-5, 300))
        assert int(block(seed, scene, frame, car, 4)[0]) == ppamd.lib.pp_sensor_word(seed, scene, frame, car)
        for q in range(4):
            a = float(ih_unit(block(seed, scene, frame, car, q)))
            assert a == ppamd.lib.pp_sensor_gauss(seed, scene, frame, car, q)
    # the stream is the sensor's own: not pp_mc_gauss's
    assert ppamd.lib.pp_sensor_gauss(9, 4, 0, 3, 1) != ppamd.lib.pp_mc_gauss(9, 4, 0, 3, 1)


def hand_scene():
    """The ego at (0, -3); ids 1, 4, 6, 9 = far (30, 0), off the line (0, 15), near (10, 0), middle
    (20, 0). Distances from the centres to the sight lines: the middle car to the far car's 30 / sqrt(909) =
    0.995 m, the near car to the far car's 60 / sqrt(909) = 1.99 m, the near car to the middle car's
    30 / sqrt(409) = 1.48 m. With a radius of 1.2 m the middle car hides the far one and nothing else is
    hidden; the fifth row is not in use."""
    sc = ppamd.alloc_scenes(1, 5)
    sc["ego_y"][0] = -3.0
    sc["n_cars"][0] = 4
    sc["car_id"][:4, 0] = [1, 4, 6, 9]
    sc["car_x"][:4, 0] = [30.0, 0.0, 10.0, 20.0]
    sc["car_y"][:4, 0] = [0.0, 15.0, 0.0, 0.0]
    sc["car_vx"][:4, 0] = [20.0, 0.0, 12.0, 15.0]
    sc["car_vy"][:4, 0] = [0.5, -1.0, 0.0, 0.25]
    sc["car_x"][4, 0] = 5.0          # garbage beyond n_cars, on every sight line: never read
    return sc


def test_hand_made_scene():
    sc = hand_scene()
    cfg = ppamd.default_sensor_cfg(seed=5, first_scene=40, pos_sigma=0.5, pos_sigma_per_m=0.01, vel_sigma=0.25,
                                   occlusion_radius=1.2)
    st = ppamd.alloc_sensor(1, 5)
    st["frame"][0] = 2
    host_sense(sc, cfg, st)
    assert st["fate"][:, 0].tolist() == [OCCLUDED, REPORTED, REPORTED, REPORTED, NONE]
    assert st["n_cars"][0] == 3 and st["frame"][0] == 3 and st["car_id"][:3, 0].tolist() == [4, 6, 9]
    for row, r in enumerate((1, 2, 3)):
        j = int(sc["car_id"][r, 0])
        g = [ppamd.lib.pp_sensor_gauss(5, 40, 2, j, q) for q in range(4)]
        rho = np.sqrt(sc["car_x"][r, 0] ** 2 + (sc["car_y"][r, 0] + 3.0) ** 2)
        sp = 0.5 + 0.01 * rho
        assert st["car_x"][row, 0] == sc["car_x"][r, 0] + sp * g[0]
        assert st["car_y"][row, 0] == sc["car_y"][r, 0] + sp * g[1]
        assert st["car_vx"][row, 0] == sc["car_vx"][r, 0] + 0.25 * g[2]
        assert st["car_vy"][row, 0] == sc["car_vy"][r, 0] + 0.25 * g[3]
        assert all(abs(x) < 2 * 3 ** 0.5 + 1e-12 for x in g)
    same_bits(used_rows(oracle(sc, cfg, np.array([2]))), used_rows(st), "oracle")
    # a smaller radius hides nothing; a dropped car still hides (every truth row can occlude)
    cfg.occlusion_radius = 0.9
    assert host_sense(sc, cfg)["fate"][:, 0].tolist() == [REPORTED] * 4 + [NONE]
    cfg.occlusion_radius, cfg.dropout_prob = 1.2, 1.0
    st = host_sense(sc, cfg)
    assert st["fate"][:, 0].tolist() == [OCCLUDED, DROPPED, DROPPED, DROPPED, NONE] and st["n_cars"][0] == 0
    # the ego on the cars' line: the near car hides both behind it, the middle one hidden itself
    sc["ego_y"][0] = 0.0
    cfg.dropout_prob = 0.0
    assert host_sense(sc, cfg)["fate"][:, 0].tolist() == [OCCLUDED, REPORTED, REPORTED, OCCLUDED, NONE]


@pytest.mark.parametrize("S", SIZES)
def test_identity_sensor(S):
    sc = random_truth(S)
    st = host_sense(sc, ppamd.default_sensor_cfg())
    live = np.arange(12)[:, None] < sc["n_cars"][None]
    assert (st["fate"] == np.where(live, REPORTED, NONE)).all()
    want = {k: np.where(live, sc[k], 0) for k in ROWS}
    want["n_cars"] = sc["n_cars"]
    same_bits(want, {k: st[k] for k in want}, "identity")
    assert (st["frame"] == 1).all()


def check_frames(sc, what):
    seen = set()
    before = to_np(sc)
    for kw in CFGS:
        cfg = ppamd.default_sensor_cfg(**kw)
        st = host_sense(sc, cfg)
        o = oracle(sc, cfg, np.zeros(len(sc["ego_x"]), np.int64))
        same_bits(o, st, f"{what} {kw}")
        seen |= set(np.unique(st["fate"]).tolist())
        # compaction in truth order: the sensed ids are the reported truth ids, ascending
        for s in range(0, len(sc["ego_x"]), 37):
            ids = sc["car_id"][st["fate"][:, s] == REPORTED, s]
            assert st["car_id"][:st["n_cars"][s], s].tolist() == ids.tolist()
    same_bits(before, to_np(sc), "truth")
    return seen


@pytest.mark.parametrize("S", SIZES)
def test_random_frames_vs_oracle(S):
    seen = check_frames(random_truth(S), f"S={S}")
    if S >= 63:
        assert seen == {NONE, REPORTED, OCCLUDED, DROPPED}


def test_hundred_car_scenes_vs_oracle():
    sc = hundred_car_truth()
    assert sc["car_id"].shape[0] == 100 and (sc["n_cars"] == 100).all()
    assert check_frames(sc, "100 cars") == {REPORTED, OCCLUDED, DROPPED}


def test_keying_deleting_a_row_changes_no_other_car():
    sc = random_truth(257)
    cfg = ppamd.default_sensor_cfg(seed=3, pos_sigma=0.5, pos_sigma_per_m=0.02, vel_sigma=0.4, dropout_prob=0.3)
    full = host_sense(sc, cfg)
    cut = to_np(sc)
    gone = 4                                           # truth row 4 of every scene that has one
    has = sc["n_cars"] > gone
    for k in ROWS:
        cut[k][gone:-1] = np.where(has, sc[k][gone + 1:], sc[k][gone:-1])
    cut["n_cars"] = sc["n_cars"] - has
    part = host_sense(cut, cfg)
    by_id = lambda st, s: {int(st["car_id"][r, s]): tuple(st[k][r, s] for k in ROWS) for r in range(st["n_cars"][s])}
    n_checked = 0
    for s in range(257):
        a, b = by_id(full, s), by_id(part, s)
        a.pop(int(sc["car_id"][gone, s]), None) if has[s] else None
        assert a == b, s
        n_checked += len(b)
    assert n_checked > 500


def test_sharding():
    sc = random_truth(1000)
    cfg = ppamd.default_sensor_cfg(**dict(CFGS[4], first_scene=7))
    whole = host_sense(sc, cfg)
    for a, b in ((0, 500), (500, 1000)):
        half = {k: np.ascontiguousarray(v[..., a:b]) for k, v in sc.items()}
        cfg.first_scene = 7 + a
        same_bits({k: v[..., a:b] for k, v in whole.items()}, host_sense(half, cfg), f"shard {a}")


def test_frames_draw_differently_and_zeroing_frame_restarts():
    sc = random_truth(65)
    cfg = ppamd.default_sensor_cfg(**CFGS[4])
    st = host_sense(sc, cfg)
    first = to_np(st)
    host_sense(sc, cfg, st)
    assert (st["frame"] == 2).all() and not np.array_equal(first["car_x"], st["car_x"])
    assert not np.array_equal(first["fate"], st["fate"])
    same_bits(used_rows(oracle(sc, cfg, np.ones(65, np.int64))), used_rows(st), "second frame")
    st["frame"][:] = 0
    host_sense(sc, cfg, st)
    same_bits(used_rows(first), used_rows(st), "restart")


def test_car_at_the_ego_position():
    """rho = 0: never occluded (nothing is nearer), sigma_p = pos_sigma, no NaN; it hides what lies
    behind it in any direction only through the other row's own sight line."""
    sc = ppamd.alloc_scenes(1, 3)
    sc["ego_x"][0], sc["ego_y"][0] = 100.0, 50.0
    sc["n_cars"][0] = 3
    sc["car_id"][:, 0] = [0, 1, 2]
    sc["car_x"][:, 0] = [100.0, 100.0, 110.0]
    sc["car_y"][:, 0] = [50.0, 50.0, 50.0]
    cfg = ppamd.default_sensor_cfg(pos_sigma_per_m=0.1, vel_sigma=0.1, occlusion_radius=2.0)
    st = host_sense(sc, cfg)
    assert st["fate"][:, 0].tolist() == [REPORTED, REPORTED, OCCLUDED] and st["n_cars"][0] == 2
    assert all(np.isfinite(st[k]).all() for k in ROWS[1:])
    assert st["car_x"][0, 0] == 100.0 and st["car_y"][1, 0] == 50.0        # sigma_p = 0.1 * 0: copied
    same_bits(used_rows(oracle(sc, cfg, np.zeros(1, np.int64))), used_rows(st), "oracle")


def test_argument_errors():
    S, R = 6, 4
    sc = ppamd.alloc_scenes(S, R)
    sc["n_cars"][:] = 3
    st = ppamd.alloc_sensor(S, R)
    for v in st.values():
        v[...] = 77
    ref = C.byref

    def call(sc_=sc, cfg=None, st_=st, device=None, **over):
        b = ppamd.scene_struct(sc_) if sc_ is not None else None
        for k, v in over.items():
            setattr(b, k, v)
        c = cfg if cfg is not None else ppamd.default_sensor_cfg()
        X = ppamd.sensor_struct(st_) if st_ is not None else None
        args = (ref(b) if b is not None else None, ref(c) if c != "null" else None, ref(X) if X is not None else None)
        if device is None:
            return ppamd.lib.pp_sense_frame_host(*args)
        return ppamd.lib.pp_sense_frame(*args, device, None)

    bad_cfgs = [dict(pos_sigma=-1.0), dict(pos_sigma=NAN), dict(pos_sigma=INF), dict(pos_sigma_per_m=-0.1),
                dict(pos_sigma_per_m=INF), dict(vel_sigma=-2.0), dict(vel_sigma=NAN), dict(occlusion_radius=-1.0),
                dict(occlusion_radius=INF), dict(occlusion_radius=NAN), dict(dropout_prob=-0.01),
                dict(dropout_prob=1.01), dict(dropout_prob=NAN), dict(first_scene=-1)]
    for device in (None, 0):
        assert call(sc_=None, device=device) == -1 and call(cfg="null", device=device) == -1
        assert call(st_=None, device=device) == -1
        for k in ("ego_x", "ego_y", "n_cars", "car_id", "car_x", "car_y", "car_vx", "car_vy"):
            assert call(device=device, **{k: None}) == -1, k
        for k in st:
            assert call(st_=dict(st, **{k: None}), device=device) == -1, k
        for kw in bad_cfgs:
            assert call(cfg=ppamd.default_sensor_cfg(**kw), device=device) == -1, kw
        assert call(device=device, n_scenes=-1) == -1 and call(device=device, car_stride=-1) == -1
        assert call(device=device, car_stride=ppamd.MAX_CARS + 1) == -1
    assert call(device=-1) == -1 and call(device=99) == -1
    assert all((v == 77).all() for v in st.values())
    # the limits themselves are fine; no scenes: nothing is written
    assert call(cfg=ppamd.default_sensor_cfg(dropout_prob=1.0, pos_sigma=0.0)) == 0
    for v in st.values():
        v[...] = 77
    assert call(n_scenes=0) == 0 and call(device=0, n_scenes=0) == 0
    assert all((v == 77).all() for v in st.values())


def test_rollout_and_sweep_argument_errors():
    """A lone sensor configuration or state, a sensor the stage would refuse (the second of two sets), no
    sensor sets: PP_ERR_ARG before anything is launched (host arrays stand in for the device buffers:
    nothing may touch them)."""
    m = env()["m"]
    S, n = 8, 12
    good = ppamd.default_params()
    sc = ppamd.add_car_table(ppamd.alloc_scenes(S, n), slots=n)
    tr, res = ppamd.alloc_traffic(S, n), ppamd.alloc_result(S, good)
    tr["n_cars"] = n
    jd, fo, lc = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n), ppamd.alloc_lane_change(S, n)
    st, se = ppamd.alloc_judge_stats(4, 8), ppamd.alloc_sensor(S, n)
    bufs = (sc, tr, res, jd, fo, lc, st, se)
    before = [to_np(d) for d in bufs]
    ref = C.byref
    b, T, R = ppamd.scene_struct(sc), ppamd.traffic_struct(tr), ppamd.result_struct(res)
    J, F, L, O = ppamd.judge_struct(jd), ppamd.follow_struct(fo), ppamd.lane_change_struct(lc), ppamd.stats_struct(st)
    X = ppamd.sensor_struct(se)
    ok = ppamd.default_sensor_cfg()

    def rollout(scfg, sstate):
        rc = ppamd.RolloutCfg(2, 3, 300.0)
        return ppamd.lib.pp_rollout_sensed(m.handle, ref(b), ref(T), ref(good), ref(rc), ref(R), None, 0, None,
                                           ref(ppamd.default_judge_cfg()), ref(J), ref(ppamd.default_follow_cfg()),
                                           ref(F), ref(ppamd.default_lane_change_cfg()), ref(L), scfg, sstate)

    assert rollout(ref(ok), None) == -1 and rollout(None, ref(X)) == -1
    assert rollout(ref(ppamd.default_sensor_cfg(dropout_prob=2.0)), ref(X)) == -1
    assert rollout(ref(ok), ref(ppamd.sensor_struct(dict(se, fate=None)))) == -1

    def sweep(sensors, sstate=True, sets=None):
        sets = sets or [good] * len(sensors or [ok])
        arr = (ppamd.Params * len(sets))(*sets)
        sarr = (ppamd.SensorCfg * len(sensors))(*sensors) if sensors else None
        cfg = ppamd.SweepCfg(len(sets), 0, 1, 0, ppamd.RolloutCfg(2, 3, 300.0), ppamd.SummaryCfg(4, 8, 0, 100.0, 0, 0))
        return ppamd.lib.pp_rollout_sweep_sensed(
            m.handle, arr, ref(cfg), ref(ppamd.default_episode_cfg()), ref(ppamd.default_judge_cfg()),
            ref(ppamd.default_follow_cfg()), ref(ppamd.default_lane_change_cfg()), ref(b), ref(T), ref(R), ref(J),
            ref(F), ref(L), ref(O), 0, None, sarr, ref(X) if sstate else None)

    assert sweep(None) == -1 and sweep([ok], sstate=False) == -1
    assert sweep([ok, ppamd.default_sensor_cfg(pos_sigma=-1.0)]) == -1
    assert sweep([ok, ppamd.default_sensor_cfg(first_scene=-4)]) == -1
    assert sweep([ok, ok], sets=[good, ppamd.default_params(n_speeds=9)]) == -1
    for d, was in zip(bufs, before):
        same_bits(was, to_np(d), "buffers")


def test_statistics_of_the_draws():
    """12,000 truth rows (1000 scenes x 12 cars, seeded). The Irwin-Hall sum of four uniforms has
    kurtosis 2.7, so the sample variance of N unit draws has standard deviation sqrt(1.7 / N); the
    dropped share of N rows sqrt(p (1 - p) / N). Both within five of those."""
    geo = env()["geo"]
    fr = random_frame(geo, 1000, 12, 99)
    sc = truth_of(geo, fr["ex"], fr["ey"], fr["traffic"])
    N = 12000
    cfg = ppamd.default_sensor_cfg(seed=2024, pos_sigma=0.3, pos_sigma_per_m=0.02)
    st = host_sense(sc, cfg)
    assert (st["n_cars"] == 12).all()
    rho = np.sqrt((sc["car_x"] - sc["ego_x"]) ** 2 + (sc["car_y"] - sc["ego_y"]) ** 2)
    z = ((st["car_x"] - sc["car_x"]) / (0.3 + 0.02 * rho)).ravel()
    assert z.size == N and abs(z.var() - 1.0) <= 5 * np.sqrt(1.7 / N), z.var()
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    p = 0.3
    st = host_sense(sc, ppamd.default_sensor_cfg(seed=2024, dropout_prob=p))
    share = (st["fate"] == DROPPED).mean()
    assert abs(share - p) <= 5 * np.sqrt(p * (1 - p) / N), share


# ---- GPU ----------------------------------------------------------------------------------------------
NOISY = dict(seed=123, pos_sigma=0.5, pos_sigma_per_m=0.01, vel_sigma=0.5, dropout_prob=0.2, occlusion_radius=1.5)


@pytest.mark.gpu
class TestSensorGPU:
    @pytest.fixture(scope="class")
    def genv(self):
        import torch
        e = env()
        return {"m": e["m"], "geo": e["geo"], "torch": torch, "dev": torch.device("cuda", 0)}

    def upload(self, genv, d):
        t = genv["torch"]
        return {k: (t.from_numpy(v).to(genv["dev"]) if isinstance(v, np.ndarray) else v) for k, v in d.items()}

    def device_check(self, genv, sc, what):
        scd = self.upload(genv, sc)
        S, R = len(sc["ego_x"]), sc["car_id"].shape[0]
        for kw in CFGS:
            cfg = ppamd.default_sensor_cfg(**kw)
            sd = ppamd.alloc_sensor(S, R, xp="torch", device=genv["dev"])
            sh = ppamd.alloc_sensor(S, R)
            for _ in range(2):                         # a fresh frame, then a carried one
                ppamd.sense_frame(scd, sd, cfg, device=0)
                host_sense(sc, cfg, sh)
                genv["torch"].cuda.synchronize()
                same_bits(sh, ppamd.sensor_to_numpy(sd), f"{what} {kw}")
        same_bits(sc, to_np(scd), "truth")

    @pytest.mark.parametrize("S", SIZES)
    def test_device_equals_host_bits(self, genv, S):
        self.device_check(genv, random_truth(S), f"S={S}")

    def test_device_equals_host_bits_hundred_cars(self, genv):
        self.device_check(genv, hundred_car_truth(), "100 cars")

    def start(self, genv, S, seed=31):
        dev, m = genv["dev"], genv["m"]
        st = {"judge": ppamd.alloc_judge(S, xp="torch", device=dev),
              "follow": ppamd.alloc_follow(S, 12, xp="torch", device=dev),
              "lane_change": ppamd.alloc_lane_change(S, 12, xp="torch", device=dev),
              "sensor": ppamd.alloc_sensor(S, 12, xp="torch", device=dev)}
        st["scenes"], st["traffic"] = ppamd.synth_episode(m, S, seed=seed, device=0, judge=st["judge"],
                                                          follow=st["follow"])
        st["result"] = ppamd.alloc_result(S, ppamd.default_params(), xp="torch", device=dev)
        return st

    def drive(self, genv, st, F, scfg=None, sensed=True, log=None):
        prm = ppamd.default_params()
        if sensed:
            ppamd.rollout_sensed(genv["m"], st["scenes"], st["traffic"], prm, st["result"], st["follow"],
                                 st["lane_change"], st["sensor"], F, 3, 300.0, judge=st["judge"], scfg=scfg, log=log)
        else:
            ppamd.rollout_lane_changing(genv["m"], st["scenes"], st["traffic"], prm, st["result"], st["follow"],
                                        st["lane_change"], F, 3, 300.0, judge=st["judge"], log=log)
        genv["torch"].cuda.synchronize()

    WORLD = ["scenes", "traffic", "result", "judge", "follow", "lane_change"]

    def same_world(self, a, b, what, keys=None):
        for k in keys or self.WORLD:
            same_bits(to_np(a[k]), to_np(b[k]), f"{what} {k}")

    def test_identity_sensor_drives_as_lane_changing(self, genv):
        S, F = 1000, 40
        plain, ident = self.start(genv, S), self.start(genv, S)
        self.drive(genv, plain, F, sensed=False)
        self.drive(genv, ident, F)
        self.same_world(plain, ident, "identity")
        se, sc = ppamd.sensor_to_numpy(ident["sensor"]), to_np(ident["scenes"])
        assert (se["frame"] == F).all() and (to_np(plain["judge"])["dist"] > 1).any()
        assert np.isin(se["fate"], (NONE, REPORTED)).all()
        assert not np.array_equal(se["car_x"], sc["car_x"])       # (the last frame's truth has moved on)

    def test_noisy_drive_frame_by_frame(self, genv):
        """20 one-frame calls of a noisy sensor over 300 scenes: each frame's sensed rows are the host
        twin's on the telemetry the frame began with, pp_eval on that telemetry with those rows gives the
        logged winner and plan and the frame's car table; one 20-frame call ends in the same bits."""
        S, F, t, m = 300, 20, genv["torch"], genv["m"]
        cfg = ppamd.default_sensor_cfg(**NOISY)
        prm = ppamd.default_params()
        step, once = self.start(genv, S), self.start(genv, S)
        hs = ppamd.alloc_sensor(S, 12)
        fates = set()
        for f in range(F):
            snap = {k: v.clone() for k, v in step["scenes"].items()}
            log = ppamd.alloc_log(1, S, prm.n_points, xp="torch", device=genv["dev"])
            self.drive(genv, step, 1, cfg, log=log)
            host_sense(to_np(snap), cfg, hs)
            se = ppamd.sensor_to_numpy(step["sensor"])
            same_bits(hs, se, f"frame {f} sensed")
            fates |= set(np.unique(se["fate"]).tolist())
            res = ppamd.alloc_result(S, prm, xp="torch", device=genv["dev"])
            ppamd.evaluate(m, ppamd.sensed_scenes(snap, step["sensor"]), prm, res, device=0)
            t.cuda.synchronize()
            got, lg = ppamd.result_to_numpy(res), to_np(log)
            same_bits({"winner": lg["winner"][0], "n_out": lg["n_out"][0], "x": lg["plan_x"][0], "y": lg["plan_y"][0]},
                      {"winner": got["winner"], "n_out": got["n_out"], "x": got["next_x"], "y": got["next_y"]},
                      f"frame {f} plan")
            tab = ppamd.TABLE_FIELDS_I + ppamd.TABLE_FIELDS_F
            same_bits({k: to_np(snap)[k] for k in tab}, {k: to_np(step["scenes"])[k] for k in tab}, f"frame {f} table")
        assert fates == {NONE, REPORTED, OCCLUDED, DROPPED} or fates == {REPORTED, OCCLUDED, DROPPED}
        self.drive(genv, once, F, cfg)
        self.same_world(step, once, "20 x 1 == 1 x 20", self.WORLD + ["sensor"])

    def test_noisy_drive_differs_and_telemetry_stays_the_truth(self, genv):
        """The telemetry after a noisy drive holds the true placements of its traffic state (the lane
        geometry restated in NumPy: within 1e-9 m, the rounding of that restatement), not the sensed
        rows; the drive is not the identity sensor's."""
        S, F, geo = 1000, 40, genv["geo"]
        ident, noisy = self.start(genv, S), self.start(genv, S)
        self.drive(genv, ident, F)
        self.drive(genv, noisy, F, ppamd.default_sensor_cfg(**NOISY))
        a, b = to_np(ident["scenes"]), to_np(noisy["scenes"])
        assert not np.array_equal(a["ego_x"], b["ego_x"]) or not np.array_equal(a["ego_y"], b["ego_y"])
        tr, se = to_np(noisy["traffic"]), ppamd.sensor_to_numpy(noisy["sensor"])
        p, u = geo.car(tr["lane"], tr["seg"], tr["t"], tr["offset"])
        d2 = (p[..., 0] - b["ego_x"]) ** 2 + (p[..., 1] - b["ego_y"]) ** 2
        sure = np.abs(np.sqrt(d2) - 300.0) > 1e-6
        n_rows = 0
        for s in range(S):
            ids = b["car_id"][:b["n_cars"][s], s]
            if sure[:, s].all():
                assert ids.tolist() == np.nonzero(d2[:, s] <= 300.0 ** 2)[0].tolist(), s
            for r, j in enumerate(ids):
                want = (p[j, s, 0], p[j, s, 1], u[j, s, 0] * tr["speed"][j, s], u[j, s, 1] * tr["speed"][j, s])
                got = tuple(b[k][r, s] for k in ROWS[1:])
                assert np.allclose(got, want, rtol=0, atol=1e-9), (s, j)
                n_rows += 1
        assert n_rows > 5 * S
        assert (se["fate"] == DROPPED).any() and not np.array_equal(se["car_x"][0], b["car_x"][0])

    def test_sweep_equals_the_calls_made_by_hand(self, genv):
        """Three sets (identity; pos_sigma 1; dropout_prob 0.5), 1,024 scenes in G = 2 groups, 30 frames."""
        S, E, F, B, hm, G = 1024, 512, 30, 64, 64.0, 2
        m, t = genv["m"], genv["torch"]
        sensors = [ppamd.default_sensor_cfg(), ppamd.default_sensor_cfg(pos_sigma=1.0),
                   ppamd.default_sensor_cfg(dropout_prob=0.5)]
        sets = [ppamd.default_params()] * 3
        stats, buf = ppamd.rollout_sweep(m, sets, S, F, scenes_per_group=E, seed=31, hist_bins=B, hist_max=hm,
                                         sensors=sensors)
        plain, _ = ppamd.rollout_sweep(m, sets[:1], S, F, scenes_per_group=E, seed=31, hist_bins=B, hist_max=hm)
        t.cuda.synchronize()
        stats, plain = to_np(stats), to_np(plain)
        assert (ppamd.sensor_to_numpy(buf["sensor"])["frame"] == F).all()
        rows = lambda p: {k: v[..., p * G:(p + 1) * G] for k, v in stats.items()}
        for p, scfg in enumerate(sensors):
            st = self.start(genv, S)
            self.drive(genv, st, F, scfg)
            hand = ppamd.judge_summary(st["judge"], S, E, hist_bins=B, hist_max=hm, m=m, device=0)
            t.cuda.synchronize()
            same_bits(to_np(hand), rows(p), f"set {p}")
        same_bits(plain, rows(0), "identity set == pp_rollout_sweep")
        for p in (1, 2):
            differ = [k for k in ("dist_sum", "clean_dist_sum", "min_sep") if not np.array_equal(rows(0)[k], rows(p)[k])]
            assert differ, f"set {p} drove exactly as the identity sensor: the sensor did not reach the planner"
