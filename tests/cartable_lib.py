"""What the car-table tests share (test_cartable.py, test_cartable_shapes.py,
golden/make_cartable_golden.py): scenes with many rows and wide ids, closed-loop episodes next to a
reference session, the host std::map restated as a Python dict over pp_scene_batch table slots, and
the two-frame table-state generator with its coverage census. A plain module beside oracle_lib.py
and world_lib.py: it holds no tests."""
import ctypes as C

import numpy as np

import oracle_lib
from oracle_lib import ppamd

I32_MAX = 2 ** 31 - 1
I32_MIN = -2 ** 31
TAB_I, TAB_F = ppamd.TABLE_FIELDS_I, ppamd.TABLE_FIELDS_F
ROW_F = ppamd.CAR_FIELDS_F
CAR_UNMATCHED = ppamd.STATUS_BITS["CAR_UNMATCHED"]


def many_car_scenes(m, S, seed, ids_fn, rows=24):
    """S synthetic scenes with `rows` sensor_fusion rows: the cars of ceil(rows / 12) generator
    batches side by side, rows reordered by the ids ids_fn(rng, rows) (ascending, as the batch
    contract requires); every 7th scene reports 5 rows fewer."""
    bs = [ppamd.synth_host(m, S, seed=seed + i, first=0) for i in range((rows + 11) // 12)]
    sc = {k: v for k, v in bs[0].items()}
    for k in ("car_x", "car_y", "car_vx", "car_vy"):
        sc[k] = np.ascontiguousarray(np.concatenate([b[k] for b in bs], 0)[:rows])
    rng = np.random.default_rng(seed)
    ids = np.zeros((rows, S), np.int32)
    for s in range(S):
        ids[:, s] = np.sort(ids_fn(rng, rows))
    sc["car_id"] = ids
    sc["n_cars"] = np.full(S, rows, np.int32)
    sc["n_cars"][::7] = rows - 5
    return sc


def ids_wide(rng, n):
    """distinct ascending ints: negatives (-1 in about half the scenes), sparse, up to 2^30"""
    pool = np.concatenate([rng.choice(np.arange(-40, 0), 3, replace=False),
                           rng.choice(np.arange(16, 2 ** 30, 9973), n, replace=False)])
    if rng.random() < 0.5:
        pool[0] = -1
    return rng.choice(np.unique(pool), n, replace=False)


# ---- closed-loop episodes next to a reference session -------------------------------------------
class Traffic:
    """Cars following lane centre polylines (map geometry), seeded; ids given. The cars drawn to
    leave do so after frame `leave_after` (60 m further off the road every frame: matching fails
    beyond 1 km)."""

    def __init__(self, geom, ids, rng, ego_s0, leave_after=40):
        self.lc = [geom[:, 4 + 2 * L:6 + 2 * L] for L in range(ppamd.NUM_LANES)]
        seg = [np.hypot(*np.diff(np.vstack([c, c[:1]]), axis=0).T) for c in self.lc]
        self.cum = [np.concatenate([[0], np.cumsum(s)]) for s in seg]
        self.ids = list(ids)
        n = len(ids)
        self.lane = rng.integers(0, ppamd.NUM_LANES, n)
        self.s = (ego_s0 + rng.uniform(-60, 260, n)) % self.cum[0][-1]
        self.v = rng.uniform(4, 26, n)
        self.off = rng.uniform(-0.4, 0.4, n)
        self.leave = rng.random(n) < 0.25           # leave the road (matching fails > 1 km off)
        self.leave_after = leave_after
        self.leave_step = 60.0

    def pos(self, j):
        L = self.lane[j]
        c, cum = self.lc[L], self.cum[L]
        s = self.s[j] % cum[-1]
        i = int(np.searchsorted(cum, s, side="right") - 1)
        a, b = c[i % len(c)], c[(i + 1) % len(c)]
        t = (s - cum[i]) / (cum[i + 1] - cum[i])
        u = (b - a) / np.hypot(*(b - a))
        p = a + t * (b - a) + self.off[j] * np.array([u[1], -u[0]])
        return p, u * self.v[j]

    def step(self, dt, f):
        self.s += self.v * dt
        self.off = np.where(self.leave & (f > self.leave_after), self.off + self.leave_step, self.off)


class Episode:
    """One closed-loop drive's world: an ego that starts on a lane centre with a previous path along
    it (a synthetic scene), Traffic with the given ids placed around it, a sensor of `sensor_range`
    metres. rows() is the frame's sensor_fusion (ascending id); drive(plan) consumes 3 points of the
    plan and moves the traffic on."""

    def __init__(self, m, ids, seed, sensor_range, leave_after=40, leave_step=60.0):
        self.rng = rng = np.random.default_rng(seed)
        sc = ppamd.synth_host(m, 1, seed=seed, first=0)
        self.ego = [float(sc["ego_x"][0]), float(sc["ego_y"][0]), float(sc["ego_yaw_deg"][0]),
                    float(sc["ego_speed_mph"][0])]
        self.prev = np.stack([sc["prev_x"][:, 0], sc["prev_y"][:, 0]], 1)[:int(sc["n_prev"][0])]
        self.traffic = traffic = Traffic(m.geometry(), ids, rng, 0.0, leave_after)
        traffic.leave_step = leave_step
        # place the traffic near the ego: shift each car's s so it starts within the sensor window
        ego_pt = np.array(self.ego[:2])
        for j in range(len(ids)):
            c, cum = traffic.lc[traffic.lane[j]], traffic.cum[traffic.lane[j]]
            k = int(np.argmin(np.hypot(*(c - ego_pt).T)))
            traffic.s[j] = (cum[k] + rng.uniform(-50, 200)) % cum[-1]
        self.sensor_range = sensor_range
        self.f = 0

    def rows(self):
        rows = []
        for j, cid in enumerate(self.traffic.ids):
            p, v = self.traffic.pos(j)
            if np.hypot(*(p - np.array(self.ego[:2]))) <= self.sensor_range:
                rows.append((cid, p[0], p[1], v[0], v[1]))
        return sorted(rows, key=lambda r: r[0])

    def shuffled(self, rows):
        """the rows in the order sent to the reference, which iterates them as they come"""
        return [rows[i] for i in self.rng.permutation(len(rows))]

    def drive(self, plan):
        n = len(plan)
        k = min(3, n)
        if k >= 1:
            q = plan[k - 2] if k >= 2 else np.array(self.ego[:2])
            d = plan[k - 1] - q
            self.ego = [plan[k - 1][0], plan[k - 1][1],
                        float(np.degrees(np.arctan2(d[1], d[0]))) if np.hypot(*d) > 0 else self.ego[2],
                        float(np.hypot(*d) * 50 * 2.237)]
        self.prev = plan[k:]
        self.traffic.step(0.02 * max(k, 1), self.f)
        self.f += 1


def ref_session_frame(rlib, h, ego, prev, rows_sent, target_lane):
    """One frame of a reference session -> (next [n, 2], target lane, entries in its std::map)."""
    one = oracle_lib.one_scene(ego, prev, rows_sent, target_lane)
    nxy = np.zeros(100)
    n_out, tl, ntab = C.c_int(), C.c_int(), C.c_int()
    with oracle_lib.quiet_stdout():
        rlib.ref_session_frame(h, C.byref(one["struct"]), nxy.ctypes.data_as(oracle_lib._dp), C.byref(n_out),
                               C.byref(tl), C.byref(ntab))
    return nxy[:2 * n_out.value].reshape(n_out.value, 2).copy(), tl.value, ntab.value


def run_episode(env, ids, frames, seed, sensor_range):
    """pp_plan_frame next to a reference session over one episode; every frame within
    oracle_lib.TOL. Returns (largest |dxy|, frames with stale entries, with erased ones, most rows
    reported)."""
    m, wx, wy = env["m"], env["wx"], env["wy"]
    rlib = env["rlib"]
    ep = Episode(m, ids, seed, sensor_range)
    ppamd.plan_reset(m)
    h = rlib.ref_session_new(oracle_lib._arr(wx), oracle_lib._arr(wy), len(wx), 1)
    tl_gpu = 1
    worst, stale, erased, reported_max = 0.0, 0, 0, 0
    try:
        for f in range(frames):
            rows = ep.rows()
            reported_max = max(reported_max, len(rows))
            # reference session (one scene, rows in any order: the reference iterates them as sent)
            rows_sent = ep.shuffled(rows)
            ref_xy, tl_ref, ntab = ref_session_frame(rlib, h, ep.ego, ep.prev, rows_sent, tl_gpu)
            nx, ny, tl_gpu = ppamd.plan_frame(m, ep.ego[0], ep.ego[1], ep.ego[2], ep.ego[3], ep.prev[:, 0],
                                              ep.prev[:, 1], rows_sent, target_lane=tl_gpu)
            n = len(ref_xy)
            assert len(nx) == n and tl_gpu == tl_ref, (f, len(nx), n, tl_gpu, tl_ref)
            if n:
                worst = max(worst, float(np.abs(np.stack([nx, ny], 1) - ref_xy).max()))
            assert worst <= oracle_lib.TOL, (f, worst)
            stale += ntab > len(rows)
            erased += ntab < len(rows)
            ep.drive(ref_xy)                              # drive 3 points of the plan
    finally:
        rlib.ref_session_free(h)
    return worst, stale, erased, reported_max


# ---- the host std::map as a Python dict over table slots (csrc/pp_cartable.h, restated) ----------
def empty_table(K, S, ids=True):
    """K poisoned empty slots per scene, as CarTable::layout(poison = true) writes a slot that holds
    no entry: invalid, lane INT32_MAX, NaN doubles; every id INT32_MAX (padding). ids False: no
    tab_id array (slot k is id k)."""
    t = {"tab_id": np.full((K, S), I32_MAX, np.int32) if ids else None,
         "tab_valid": np.zeros((K, S), np.int32), "tab_lane": np.full((K, S), I32_MAX, np.int32)}
    t.update({k: np.full((K, S), np.nan) for k in TAB_F})
    return t


def dict_layout(cars, ids, tab, s):
    """Scene s's slots from `cars` ({id: (lane, s, d, vs, vd, vx, vy)}) and the frame's ids: the
    union of the stored and the reported ids ascending, a stored id's slot valid with its state, any
    other slot empty (poisoned), padding (id INT32_MAX, empty) to the end. Returns the union size."""
    u = sorted(set(cars) | set(int(i) for i in ids))
    K = tab["tab_valid"].shape[0]
    assert len(u) <= K, (len(u), K)
    for k in range(K):
        tab["tab_id"][k, s] = u[k] if k < len(u) else I32_MAX
        e = cars.get(u[k]) if k < len(u) else None
        tab["tab_valid"][k, s] = e is not None
        tab["tab_lane"][k, s] = e[0] if e else I32_MAX
        for i, name in enumerate(TAB_F):
            tab[name][k, s] = e[1 + i] if e else np.nan
    return len(u)


def dict_take_back(cars, tab, s, n_used):
    """After the frame: a valid slot sets its id's entry, an invalid one erases it."""
    for k in range(n_used):
        cid = int(tab["tab_id"][k, s])
        if tab["tab_valid"][k, s]:
            cars[cid] = (int(tab["tab_lane"][k, s]),) + tuple(float(tab[name][k, s]) for name in TAB_F)
        else:
            cars.pop(cid, None)


# ---- recorded episodes: telemetry and the reference session's answers ---------------------------
EPISODES, EP_FRAMES, EP_SLOTS = 12, 25, 33


def episode_ids(e):
    """Episode e's car ids: 3 to 30 of them, sparse, negative ones and -1 among them, INT32_MIN
    and 2^31 - 2 in some."""
    rng = np.random.default_rng(9100 + e)
    n = [3, 30, 17, 16, 8, 24, 5, 29, 12, 20, 15, 27][e % 12]
    pool = {-1}
    if e % 3 == 0:
        pool.add(I32_MIN)
    if e % 4 == 1:
        pool.add(I32_MAX - 1)
    pool |= set(int(v) for v in rng.choice(np.arange(-60, -1), min(n // 3, 6, n - len(pool)), replace=False))
    while len(pool) < n:
        pool.add(int(rng.integers(0, 40)) if rng.random() < 0.3 else int(rng.integers(40, I32_MAX - 1)))
    return sorted(pool)


def record_episodes(m, wx, wy, rlib):
    """EPISODES closed-loop drives of EP_FRAMES frames, each beside its own reference session that
    plans it (rows sent in shuffled order). Returns the record the fixture stores: per episode and
    frame the telemetry (ego, the first 10 previous points and their count, the rows as sent, the
    target lane going in) and the session's outputs (next, n_out, target lane, entries in its map)."""
    E, F, R = EPISODES, EP_FRAMES, 30
    rec = {"ego": np.zeros((E, F, 4)), "prev": np.zeros((E, F, 10, 2)), "n_prev": np.zeros((E, F), np.int32),
           "tl_in": np.zeros((E, F), np.int32), "n_rows": np.zeros((E, F), np.int32),
           "row_id": np.zeros((E, F, R), np.int32), "row_xyv": np.zeros((E, F, R, 4)),
           "ref_next": np.zeros((E, F, 50, 2)), "ref_n_out": np.zeros((E, F), np.int32),
           "ref_tl": np.zeros((E, F), np.int32), "ref_n_table": np.zeros((E, F), np.int32)}
    for e in range(E):
        ids = episode_ids(e)
        assert len(ids) <= R
        ep = Episode(m, ids, 400 + e, [45.0, 1e5, 80.0, 60.0][e % 4], leave_after=5, leave_step=150.0)
        h = rlib.ref_session_new(oracle_lib._arr(wx), oracle_lib._arr(wy), len(wx), 1)
        tl = 1
        try:
            for f in range(F):
                sent = ep.shuffled(ep.rows())
                rec["ego"][e, f] = ep.ego
                n = min(len(ep.prev), 10)
                rec["prev"][e, f, :n] = ep.prev[:n]
                rec["n_prev"][e, f] = len(ep.prev)
                rec["tl_in"][e, f] = tl
                rec["n_rows"][e, f] = len(sent)
                for j, r in enumerate(sent):
                    rec["row_id"][e, f, j] = r[0]
                    rec["row_xyv"][e, f, j] = r[1:]
                xy, tl, ntab = ref_session_frame(rlib, h, ep.ego, ep.prev, sent, tl)
                rec["ref_next"][e, f, :len(xy)] = xy
                rec["ref_n_out"][e, f], rec["ref_tl"][e, f], rec["ref_n_table"][e, f] = len(xy), tl, ntab
                ep.drive(xy)
        finally:
            rlib.ref_session_free(h)
    return rec


def check_oracle_table_batch(olib, wx, wy, rec):
    """The recorded episodes as ONE oracle batch of EPISODES scenes in car-table mode, frame by
    frame: a dict per scene plays the reference's std::map, laid out over EP_SLOTS slots before the
    frame and taken back after it; rows ascending. Every scene's next_x/next_y must equal its
    session's frame exactly, n_out and the target lane too, and the dict must hold as many entries
    as the session's map. Returns a census: frames with stale entries, entries erased, largest
    union."""
    E, F = rec["n_rows"].shape
    K = R = EP_SLOTS
    prm = ppamd.default_params(n_speeds=1)
    cars = [dict() for _ in range(E)]
    census = {"stale": 0, "erased": 0, "union": 0, "minus1": 0}
    for f in range(F):
        b = ppamd.alloc_scenes(E, R)
        for k in ROW_F:
            b[k][:] = np.nan                              # rows beyond n_cars are never cars
        b.update(empty_table(K, E))
        used = []
        for e in range(E):
            b["ego_x"][e], b["ego_y"][e], b["ego_yaw_deg"][e], b["ego_speed_mph"][e] = rec["ego"][e, f]
            b["prev_x"][:, e], b["prev_y"][:, e] = rec["prev"][e, f, :, 0], rec["prev"][e, f, :, 1]
            b["n_prev"][e] = rec["n_prev"][e, f]
            b["prev_target_lane"][e] = rec["tl_in"][e, f]
            n = int(rec["n_rows"][e, f])
            order = np.argsort(rec["row_id"][e, f, :n], kind="stable")
            b["n_cars"][e] = n
            b["car_id"][:n, e] = rec["row_id"][e, f, order]
            for i, k in enumerate(ROW_F):
                b[k][:n, e] = rec["row_xyv"][e, f, order, i]
            used.append(dict_layout(cars[e], b["car_id"][:n, e], b, e))
            census["union"] = max(census["union"], used[-1])
        got = oracle_lib.oracle_eval(olib, wx, wy, b, prm, info=True)
        for e in range(E):
            before = set(cars[e])
            dict_take_back(cars[e], b, e, used[e])
            n = int(rec["ref_n_out"][e, f])
            assert got["n_out"][e] == n, (e, f, got["n_out"][e], n)
            assert got["winner"][e] // prm.n_speeds == rec["ref_tl"][e, f] == got["info"]["target_lane"][e], (e, f)
            assert np.array_equal(got["next_x"][:n, e], rec["ref_next"][e, f, :n, 0]), (e, f)
            assert np.array_equal(got["next_y"][:n, e], rec["ref_next"][e, f, :n, 1]), (e, f)
            assert len(cars[e]) == rec["ref_n_table"][e, f], (e, f, len(cars[e]), rec["ref_n_table"][e, f])
            rep = set(int(i) for i in rec["row_id"][e, f, :int(rec["n_rows"][e, f])])
            census["stale"] += len(set(cars[e]) - rep) > 0
            census["erased"] += len((before | rep) - set(cars[e]))
            census["minus1"] += -1 in cars[e]
    return census


# ---- two consecutive frames of table state for pp_eval ------------------------------------------
def _slot_ids(rng, u, K, s):
    """u distinct ascending ids: -1 in two scenes of three, INT32_MIN, 0, 2^31 - 2 and (below K
    cars) INT32_MAX as a real car's id in some, small negatives, sparse positives."""
    special = [-1] if s % 3 != 0 else []
    for v, p in ((I32_MIN, 0.3), (0, 0.5), (I32_MAX - 1, 0.3)):
        if rng.random() < p:
            special.append(v)
    if u < K and rng.random() < 0.4:
        special.append(I32_MAX)
    special = special[:u]
    need = u - len(special)
    nneg = int(rng.integers(0, min(need, 3) + 1))
    neg = rng.choice(np.arange(-40, -1), nneg, replace=False)
    pos = 1 + 9973 * rng.choice((I32_MAX - 2) // 9973, need - nneg, replace=False)
    ids = np.sort(np.concatenate([np.array(special, np.int64), neg, pos]))
    assert len(np.unique(ids)) == u
    return ids.astype(np.int32)


def table_frames(m, S, K, R, seed, ids=True):
    """Two consecutive frames of a host batch of S scenes in car-table mode: tab_slots = K,
    car_stride = R >= K (NumPy only; the cars' physical states are those of ceil(K / 12)
    ppamd.synth_host batches side by side, car k of a scene in its slot k).

    Scene s has u[s] cars (0..K, both ends occur) with the ids of _slot_ids in its first u slots
    and padding (id INT32_MAX, empty) behind them; ids False: no tab_id array, slot k is id k.
    Frame 1: an empty poisoned table (empty_table); about 70 % of the cars reported. Frame 2: the
    cars 0.06 s further on; each car reported again, not reported (stale), reported more than 1 km
    off the road (erased), or reported for the first time; some scenes report nothing, some
    everything; with K >= 17 and S >= 20, scenes 1..19 report exactly 0..18 cars. Rows ascend by id;
    rows at and beyond n_cars hold NaN positions and real slot ids. Frame 2's table state is a
    placeholder (empty): with_table() puts the table after frame 1 there.
    Returns [frame1, frame2] (host batch dicts)."""
    assert R >= K
    rng = np.random.default_rng([seed, S, K])
    bs = [ppamd.synth_host(m, S, seed=seed * 131 + i, first=0) for i in range(max((K + 11) // 12, 1))]
    phys = {k: np.concatenate([b[k] for b in bs], 0)[:K].copy() for k in ROW_F}
    u = rng.integers(0, K + 1, S)
    u[0], u[S - 1] = 0, K
    forced = K >= 17 and S >= 20                          # scenes 1..19: 0..18 rows in frame 2
    if forced:
        u[1:20] = np.maximum(u[1:20], np.minimum(np.arange(19), K))
    tid = np.full((K, S), I32_MAX, np.int32)
    for s in range(S):
        tid[:u[s], s] = _slot_ids(rng, int(u[s]), K, s) if ids else np.arange(u[s])
    if not ids:
        tid[:] = np.arange(K)[:, None]
    live = np.arange(K)[:, None] < u[None, :]
    rep1 = live & (rng.random((K, S)) < 0.7)
    c = rng.random((K, S))
    # reported in frame 1: again 40 %, stale 35 %, displaced 25 %; not: first 50 %, displaced at
    # its first report 15 %, never reported 35 %
    rep2 = live & np.where(rep1, (c < 0.4) | (c >= 0.75), c < 0.65)
    off2 = live & np.where(rep1, c >= 0.75, (c >= 0.5) & (c < 0.65))
    sc = np.arange(S)
    rep2[:, sc % 11 == 5] = False                         # nothing reported over a stale table
    rep2[:, sc % 8 == 7] = live[:, sc % 8 == 7]           # everything reported
    off2[:, sc % 8 == 7] = False
    if forced:
        for t in range(19):
            pick = rng.permutation(int(u[1 + t]))[:min(t, K)]
            rep2[:, 1 + t] = False
            rep2[pick, 1 + t] = True
    off2 &= rep2
    frames = []
    for f, rep in enumerate((rep1, rep2)):
        b = {k: v.copy() for k, v in bs[0].items() if not k.startswith("car_")}
        x = {k: phys[k].copy() for k in ROW_F}
        if f == 1:
            x["car_x"] += 0.06 * x["car_vx"]
            x["car_y"] += 0.06 * x["car_vy"]
            x["car_x"][off2] += 9000.0                    # more than 1 km from every lane segment
        b["car_id"] = np.zeros((R, S), np.int32)
        for k in ROW_F:
            b[k] = np.full((R, S), np.nan)
        b["n_cars"] = rep.sum(0).astype(np.int32)
        for s in range(S):
            sel = np.nonzero(rep[:, s])[0]
            n = len(sel)
            b["car_id"][:n, s] = tid[sel, s]
            for k in ROW_F:
                b[k][:n, s] = x[k][sel, s]
            # garbage rows: real slot ids (the last reported id first), NaN positions
            b["car_id"][n:, s] = tid[(np.arange(n, R) - 1) % K, s] if u[s] or not ids else 0
        b.update(empty_table(K, S, ids))
        if ids:
            b["tab_id"] = tid.copy()
        frames.append(b)
    return frames


def with_table(batch, table):
    """A copy of the batch with the table state (valid, lane, doubles) of `table`."""
    b = {k: (None if v is None else v.copy()) for k, v in batch.items()}
    for k in TAB_I[1:] + TAB_F:
        b[k] = table[k].copy()
    return b


def slot_view(b):
    """(slot ids [K, S]; reported [K, S]: a row of the frame carries the slot's id), from the batch
    alone. A slot that repeats its predecessor's id is padding and never reported."""
    K, S = b["tab_valid"].shape
    tid = b["tab_id"] if b.get("tab_id") is not None else np.broadcast_to(np.arange(K, dtype=np.int32)[:, None], (K, S))
    first = np.ones((K, S), bool)
    first[1:] = tid[1:] != tid[:-1]
    rep = np.zeros((K, S), bool)
    for s in range(S):
        rep[:, s] = first[:, s] & np.isin(tid[:, s], b["car_id"][:b["n_cars"][s], s])
    return tid, rep


def oracle_frames(olib, wx, wy, frames, prm):
    """The oracle over both frames, frame 2 from its own table after frame 1. Returns per frame
    (input batch, oracle result with info, table after the call)."""
    out, table = [], None
    for b in frames:
        inp = with_table(b, table) if table is not None else b
        run = {k: (None if v is None else v.copy()) for k, v in inp.items()}
        res = oracle_lib.oracle_eval(olib, wx, wy, run, prm, info=True)
        table = {k: run[k] for k in TAB_I + TAB_F}
        out.append((inp, res, table))
    return out


def coverage(ora):
    """What the two frames really exercise, counted from the oracle's results: frame 2's slot
    classes, unmatched cars, the -1 sentinel beside a matched car of id -1, in-lane follow cars that
    are stale slots and ones reported this frame, the row counts that occur, the union sizes."""
    (b1, r1, t1), (b2, r2, t2) = ora
    tid, rep = slot_view(b2)
    before, after = b2["tab_valid"] != 0, t2["tab_valid"] != 0
    K, S = before.shape
    cov = {"again": int((before & rep & after).sum()), "stale": int((before & ~rep & after).sum()),
           "erased": int((before & rep & ~after).sum()), "first": int((~before & rep & after).sum()),
           "unmatched": int(((r1["status"] | r2["status"]) & CAR_UNMATCHED != 0).sum()),
           "empty_over_stale": int(((b2["n_cars"] == 0) & (before.sum(0) > 0)).sum()),
           "all_reported": int(((before.sum(0) > 0) & (~before | rep).all(0) & (b2["n_cars"] > before.sum(0))).sum()),
           "n_cars": sorted(set(b1["n_cars"].tolist()) | set(b2["n_cars"].tolist())),
           "minus1_scenes": int(((tid == -1) & rep).any(0).sum())}
    minus1 = stale_follow = fresh_follow = 0
    for r, t, b in ((r1, t1, b1), (r2, t2, b2)):
        i, rp = slot_view(b)
        ok = t["tab_valid"] != 0
        il = r["info"]["in_lane_car"]
        minus1 += int(((il == -1) & ((i == -1) & ok).any(0)).sum())
        hit = ok & (i == il[None, :]) & (il != -1)[None, :]
        stale_follow += int((hit & ~rp).any(0).sum())
        fresh_follow += int((hit & rp).any(0).sum())
    cov.update(minus1_sentinel=minus1, follow_stale=stale_follow, follow_reported=fresh_follow)
    if b2.get("tab_id") is not None:
        pad = (tid == I32_MAX) & (b2["tab_valid"] == 0) & ~rep
        cov["u"] = sorted(set((K - pad.sum(0)).tolist()))
        cov["real_int32_max"] = int(((tid == I32_MAX) & rep).any(0).sum())
    return cov


def assert_coverage(cov, S, K, ids=True):
    """The conditions a table_frames batch must meet; the callers choose seeds at which they hold.
    (The row counts 0..18 are G - 1, G and G + 1 for every K1 group size G; a scene reports at most
    its K slots' cars, so K = 17 ends at 17, and 19 counts need 20 scenes. A scene of one slot that
    reports everything reports no more than it stored.)"""
    for k in ("again", "stale", "erased", "first", "unmatched", "empty_over_stale", "follow_stale",
              "follow_reported"):
        assert cov[k] > 0, (k, cov)
    if K > 1:
        assert cov["all_reported"] > 0, cov
    if ids:
        assert cov["minus1_sentinel"] > 0, cov
        assert 0 in cov["u"] and K in cov["u"], cov
        assert K == 1 or cov["real_int32_max"] > 0, cov
    if K >= 17 and S >= 20:
        assert set(range(min(K, 18) + 1)) <= set(cov["n_cars"]), cov
