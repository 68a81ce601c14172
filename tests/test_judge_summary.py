"""The judge summary (pp_judge_summary, pp_judge_summary_host; DESIGN.md "Judge summary and parameter
sweeps") and the parameter sweep built on it (pp_rollout_sweep).

The oracle is an independent NumPy restatement of the definitions in include/pp.h: boolean masks per
group, np.bincount for the histogram, math.fsum (exactly rounded) for the two sums. Integer figures,
bins, minima and maxima must agree exactly. The library's sums are one fixed expression: per 256-scene
tile a pairwise tree of depth 8, the tiles dealt round-robin onto 256 running sums (ceil(tiles / 256)
additions each, one more from the +0.0 they start at), then a tree of depth 8 over those: every term
passes through at most 17 + ceil(tiles / 256) additions, each with a relative error of at most 2^-53,
so for non-negative terms |sum - exact| <= (17 + ceil(tiles / 256)) 2^-53 exact to first order. That
is the bound asserted (the tests' dist and clean_dist are non-negative, as the judge's are).

CPU: host twin vs the oracle (a hand-made state with every figure worked out; seeded random states
with unjudged scenes holding garbage, NaN and +-inf in dist / clean_dist, NaN in the maxima, +inf and
NaN separations), bin edges, group independence, out_first / out_stride, every argument error,
stats_quantile. GPU: device == host bits at the tile, wave and group edges, after a real rollout, the
state untouched, two calls identical, and the sweep against its four calls made by hand."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import same_bits, to_np

K = len(ppamd.INC_KINDS)
INF, NAN = float("inf"), float("nan")
SIZES = [1, 255, 256, 257, 1000, 65537]


# ---- states -----------------------------------------------------------------------------------------
_STATES = {}


def random_state(S, seed=2026):
    """A judge state of S scenes: one in nine unjudged and full of garbage; of the judged ones a few
    with NaN or +-inf in dist or clean_dist, NaN in a maximum, a NaN or +inf separation; distances up
    to 3,000 m (beyond the histograms' 2,000), some exactly on bin edges. Made once per S and shared:
    nothing writes to it (the tests check that)."""
    if (S, seed) in _STATES:
        return _STATES[S, seed]
    rng = np.random.default_rng(seed + S)
    j = ppamd.alloc_judge(S)
    j["steps"][:] = rng.integers(1, 5000, S)
    j["count"][:] = np.where(rng.random((K, S)) < 0.3, rng.integers(1, 400, (K, S)), 0)
    j["first_step"][:] = np.where(j["count"] > 0, rng.integers(1, 5000, (K, S)), 0)
    j["flags"][:] = ((j["count"] > 0) * (1 << np.arange(K))[:, None]).sum(0).astype(np.uint32)
    j["dist"][:] = rng.uniform(0, 3000, S)
    j["clean_dist"][:] = j["dist"] * rng.random(S)
    edge = rng.random(S) < 0.05
    j["clean_dist"][edge] = rng.integers(0, 80, edge.sum()) * 31.25       # multiples of 2000 / 64
    j["dist"][edge] = np.maximum(j["dist"][edge], j["clean_dist"][edge])
    j["min_sep"][:] = np.where(rng.random(S) < 0.2, INF, rng.uniform(-2, 50, S))
    for k in ("max_speed_mph", "max_acc", "max_jerk"):
        j[k][:] = rng.uniform(0, 60, S)
    for k, share in (("dist", 0.01), ("clean_dist", 0.01), ("min_sep", 0.02), ("max_acc", 0.02), ("max_jerk", 0.02)):
        bad = rng.random(S) < share
        j[k][bad] = rng.choice([NAN, INF, -INF] if k in ("dist", "clean_dist") else [NAN], bad.sum())
    un = rng.random(S) < 1 / 9
    j["steps"][un] = 0
    for k in ("dist", "clean_dist", "min_sep", "max_speed_mph", "max_acc", "max_jerk"):
        j[k][un] = rng.choice([NAN, 1e300, -5.0], un.sum())
    j["count"][:, un] = 2 ** 31 - 1
    j["first_step"][:, un] = 1
    j["flags"][un] = 0
    _STATES[S, seed] = j
    return j


def slice_state(j, a, b):
    return {k: np.ascontiguousarray(v[..., a:b]) for k, v in j.items()}


# ---- the oracle -------------------------------------------------------------------------------------
def oracle(j, S, E, B, hist_max):
    """Rows of exact figures; the sums as math.fsum, with `tiles` per row for the bound."""
    G = -(-S // E)
    o = {k: np.zeros((G,) if lead is None else (B if lead == "b" else lead, G), dt)
         for k, dt, lead in ppamd.STATS_FIELDS}
    o["tiles"] = np.zeros(G, np.int64)
    inv_w = B / hist_max
    for g in range(G):
        sl = slice(g * E, min(S, (g + 1) * E))
        steps = j["steps"][sl].astype(np.int64)
        dist, clean = j["dist"][sl], j["clean_dist"][sl]
        judged = steps != 0
        fin = judged & np.isfinite(dist) & np.isfinite(clean)
        o["n_scenes"][g] = len(steps)
        o["tiles"][g] = -(-len(steps) // 256)
        o["n_unjudged"][g] = (~judged).sum()
        o["n_nonfinite"][g] = (judged & ~fin).sum()
        o["n_clean"][g] = (judged & (j["flags"][sl] == 0)).sum()
        o["steps"][g] = steps[judged].sum()
        for k in range(K):
            cnt, fs = j["count"][k, sl].astype(np.int64), j["first_step"][k, sl]
            o["scenes_with"][k, g] = (judged & (cnt > 0)).sum()
            o["steps_in"][k, g] = cnt[judged].sum()
            seen = fs[judged & (fs > 0)]
            o["first_step_min"][k, g] = seen.min() if len(seen) else 0
        o["dist_sum"][g] = math.fsum(dist[fin])
        o["clean_dist_sum"][g] = math.fsum(clean[fin])
        o["clean_dist_min"][g] = clean[fin].min() if fin.any() else INF
        o["clean_dist_max"][g] = clean[fin].max() if fin.any() else -INF
        sep = j["min_sep"][sl][judged]
        sep = sep[~np.isnan(sep)]
        o["min_sep"][g] = sep.min() if len(sep) else INF
        for k in ("max_speed_mph", "max_acc", "max_jerk"):
            v = j[k][sl][judged]
            v = v[~np.isnan(v)]
            o[k][g] = v.max() if len(v) else -INF
        q = clean[fin] * inv_w
        b = np.where(q >= B - 1, B - 1, np.where(q > 0, q, 0).astype(np.int64))
        o["hist"][:, g] = np.bincount(b, minlength=B)
    return o


SUMS = ("dist_sum", "clean_dist_sum")


def check_against_oracle(st, o, what=""):
    for k, _, _ in ppamd.STATS_FIELDS:
        if k in SUMS:
            bound = (17 + -(-o["tiles"] // 256)) * 2.0 ** -53 * o[k]
            err = np.abs(st[k] - o[k])
            print(f"{what} {k}: max |err| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all(), f"{what} {k}"
        else:
            assert st[k].dtype == o[k].dtype and np.array_equal(st[k], o[k]), f"{what} {k}"


def host_summary(j, S, E, B=64, hist_max=2000.0, **kw):
    return ppamd.judge_summary(j, S, E, hist_bins=B, hist_max=hist_max, host=True, **kw)


# ---- CPU: the host twin ------------------------------------------------------------------------------
def hand_state():
    """S = 5: scene 1 unjudged (garbage), scene 4 with a NaN dist."""
    j = ppamd.alloc_judge(5)
    j["steps"][:] = [90, 0, 150, 64, 30]
    j["flags"][:] = [0, 0, 0b00101, 0b10000, 0]
    j["count"][0] = [0, 99, 4, 0, 0]
    j["count"][2] = [0, 99, 7, 0, 0]
    j["count"][4] = [0, 99, 0, 11, 0]
    j["first_step"][0] = [0, 1, 80, 0, 0]
    j["first_step"][2] = [0, 1, 66, 0, 0]
    j["first_step"][4] = [0, 1, 0, 70, 0]
    j["dist"][:] = [10.5, NAN, 20.25, 3.0, NAN]
    j["clean_dist"][:] = [10.5, 1e300, 8.0, 0.0, 2.0]
    j["min_sep"][:] = [INF, -1.0, -0.25, 4.0, INF]
    j["max_speed_mph"][:] = [44.0, 1e300, 51.0, 12.0, 30.0]
    j["max_acc"][:] = [3.0, NAN, 9.0, 1.0, NAN]
    j["max_jerk"][:] = [2.0, NAN, 12.0, 0.5, 5.0]
    return j


def test_hand_made_state():
    """S = 5, E = 2: three groups, the last one short; B = 4 over [0, 16)."""
    j = hand_state()
    before = to_np(j)
    st = host_summary(j, 5, 2, B=4, hist_max=16.0)
    want = {
        "n_scenes": [2, 2, 1], "n_unjudged": [1, 0, 0], "n_nonfinite": [0, 0, 1], "n_clean": [1, 0, 1],
        "steps": [90, 214, 30],
        "scenes_with": [[0, 1, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]],
        "steps_in": [[0, 4, 0], [0, 0, 0], [0, 7, 0], [0, 0, 0], [0, 11, 0]],
        "first_step_min": [[0, 80, 0], [0, 0, 0], [0, 66, 0], [0, 0, 0], [0, 70, 0]],
        "dist_sum": [10.5, 23.25, 0.0], "clean_dist_sum": [10.5, 8.0, 0.0],
        "clean_dist_min": [10.5, 0.0, INF], "clean_dist_max": [10.5, 8.0, -INF],
        "min_sep": [INF, -0.25, INF], "max_speed_mph": [44.0, 51.0, 30.0], "max_acc": [3.0, 9.0, -INF],
        "max_jerk": [2.0, 12.0, 5.0],
        "hist": [[0, 1, 0], [0, 0, 0], [1, 1, 0], [0, 0, 0]],          # 10.5 -> bin 2; 8.0 -> 2, 0.0 -> 0
    }
    for k, dt, _ in ppamd.STATS_FIELDS:
        assert st[k].dtype == np.dtype(dt)
        assert np.array_equal(st[k], np.array(want[k], dt)), k
    same_bits(before, to_np(j), "state")
    check_against_oracle(st, oracle(j, 5, 2, 4, 16.0), "hand")


@pytest.mark.parametrize("S", SIZES)
def test_random_states_vs_oracle(S):
    j = random_state(S)
    before = to_np(j)
    for E in (1, 7, 256, 257, 1000, S):
        if E < 256 and S > 1000:
            continue
        for B, hist_max in ((64, 2000.0), (1, 5.0), (1024, 1999.0)):
            st = host_summary(j, S, E, B=B, hist_max=hist_max)
            o = oracle(j, S, E, B, hist_max)
            check_against_oracle(st, o, f"S={S} E={E} B={B}")
            judged = st["n_scenes"] - st["n_unjudged"]
            assert np.array_equal(st["hist"].sum(0), judged - st["n_nonfinite"])
            assert st["n_scenes"].sum() == S
    same_bits(before, to_np(j), "state")


def test_unjudged_garbage_changes_nothing_else():
    S = 1000
    j = random_state(S)
    clean = {k: v.copy() for k, v in j.items()}
    un = j["steps"] == 0
    assert un.sum() > 50
    for k, v in clean.items():
        if k != "steps":
            v[..., un] = 0
    a, b = host_summary(j, S, 100), host_summary(clean, S, 100)
    same_bits(a, b, "garbage")
    assert a["n_unjudged"].sum() == un.sum()


def test_bin_edges():
    """B = 4 over [0, 4): 0 and just below 1 in bin 0, exactly 1, 2, 3 in their own bins, at and beyond
    hist_max in the last one."""
    vals = [0.0, math.nextafter(1.0, 0.0), 1.0, 2.0, math.nextafter(3.0, 0.0), 3.0, math.nextafter(4.0, 0.0), 4.0,
            5.0, 1e300]
    j = ppamd.alloc_judge(len(vals))
    j["steps"][:] = 1
    j["clean_dist"][:] = vals
    j["dist"][:] = vals
    st = host_summary(j, len(vals), len(vals), B=4, hist_max=4.0)
    assert st["hist"][:, 0].tolist() == [2, 1, 2, 5]
    assert st["n_nonfinite"][0] == 0 and st["clean_dist_max"][0] == 1e300


def test_non_finite_and_all_infinite_separation():
    j = ppamd.alloc_judge(6)
    j["steps"][:] = 5
    j["dist"][:] = [1.0, NAN, INF, 2.0, 3.0, -INF]
    j["clean_dist"][:] = [1.0, 1.0, 1.0, NAN, 3.0, 0.5]
    j["min_sep"][:] = INF
    st = host_summary(j, 6, 6, B=8, hist_max=8.0)
    assert st["n_nonfinite"][0] == 4 and st["hist"][:, 0].sum() == 2
    assert st["dist_sum"][0] == 4.0 and st["clean_dist_sum"][0] == 4.0
    assert st["clean_dist_min"][0] == 1.0 and st["clean_dist_max"][0] == 3.0
    assert st["min_sep"][0] == INF and st["steps"][0] == 30 and st["n_clean"][0] == 6


@pytest.mark.parametrize("S,E", [(1000, 7), (1000, 256), (1000, 257), (65537, 1000), (65537, 30000)])
def test_group_independence(S, E):
    """Each group's row equals the summary of that slice alone, bit for bit."""
    j = random_state(S)
    st = host_summary(j, S, E)
    G = -(-S // E)
    for g in sorted({0, 1, G // 2, G - 1}):
        a, b = g * E, min(S, (g + 1) * E)
        one = host_summary(slice_state(j, a, b), b - a, b - a)
        same_bits({k: v[..., g:g + 1] for k, v in st.items()}, one, f"group {g}")


def test_out_first_and_stride_leave_other_rows():
    S, E, B = 1000, 300, 16
    j = random_state(S)
    plain = host_summary(j, S, E, B=B)
    G, R, first = 4, 9, 2
    st = ppamd.alloc_judge_stats(R, B)
    for k, v in st.items():
        v[...] = 77
    host_summary(j, S, E, B=B, stats=st, out_first=first)
    for k, v in st.items():
        assert np.array_equal(v[..., first:first + G], plain[k]), k
        rest = np.delete(v, np.s_[first:first + G], axis=-1)
        assert (rest == 77).all(), k


def _call(j, S, cfg, st, m=None, device=None):
    J, O = ppamd.judge_struct(j), ppamd.stats_struct(st)
    if device is None:
        return ppamd.lib.pp_judge_summary_host(C.byref(J) if j is not None else None, S, cfg,
                                               C.byref(O) if st is not None else None)
    return ppamd.lib.pp_judge_summary(m, C.byref(J), S, cfg, C.byref(O), device, None)


def test_argument_errors():
    S = 10
    j, st = ppamd.alloc_judge(S), ppamd.alloc_judge_stats(8, 4)
    for v in st.values():
        v[...] = 55
    cfg = lambda E=5, B=4, hm=10.0, first=0, stride=0: C.byref(ppamd.SummaryCfg(E, B, 0, hm, first, stride))
    assert _call(j, S, cfg(), st) == 0
    assert _call(j, S, None, st) == -1
    assert ppamd.lib.pp_judge_summary_host(None, S, cfg(), C.byref(ppamd.stats_struct(st))) == -1
    assert ppamd.lib.pp_judge_summary_host(C.byref(ppamd.judge_struct(j)), S, cfg(), None) == -1
    for k in j:                                        # every state array, the carried ones included
        assert _call(dict(j, **{k: None}), S, cfg(), st) == -1, k
    for k in st:
        assert _call(j, S, cfg(), dict(st, **{k: None})) == -1, k
    for bad in (cfg(E=0), cfg(E=-3), cfg(B=0), cfg(B=1025), cfg(hm=0.0), cfg(hm=-1.0), cfg(hm=NAN), cfg(hm=INF),
                cfg(first=-1, stride=8), cfg(first=1, stride=0), cfg(stride=1), cfg(first=7, stride=8),
                cfg(first=3, stride=4)):
        assert _call(j, S, bad, st) == -1
    assert _call(j, -1, cfg(), st) == -1
    assert _call(j, S, cfg(B=1024), ppamd.alloc_judge_stats(2, 1024)) == 0
    assert _call(j, S, cfg(first=6, stride=8), st) == 0
    # S == 0: fine, and nothing is written
    for v in st.values():
        v[...] = 55
    assert _call(j, 0, cfg(), st) == 0 and _call(j, 0, cfg(first=8, stride=8), st) == 0
    assert all((v == 55).all() for v in st.values())
    # the device entry point: the same checks, a NULL map and a bad device, all before any HIP call
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    assert _call(j, S, cfg(), st, None, 0) == -1
    assert _call(j, S, cfg(), st, m.handle, -1) == -1 and _call(j, S, cfg(), st, m.handle, 99) == -1
    assert _call(j, S, cfg(B=0), st, m.handle, 0) == -1 and _call(j, -1, cfg(), st, m.handle, 0) == -1
    assert _call(dict(j, dist=None), S, cfg(), st, m.handle, 0) == -1
    assert _call(j, 0, cfg(), st, m.handle, 0) == 0
    assert all((v == 55).all() for v in st.values())


def test_sweep_argument_errors():
    """n_sets < 1, a NULL argument, a set the rollout or pp_eval would refuse (the second of two), a
    lone lane-change state: PP_ERR_ARG before anything is launched (host arrays stand in for the
    device buffers: nothing may touch them)."""
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    S, n = 8, 12
    good = ppamd.default_params()
    sc = ppamd.add_car_table(ppamd.alloc_scenes(S, n), slots=n)
    tr, res = ppamd.alloc_traffic(S, n), ppamd.alloc_result(S, good)
    jd, fo, lc = ppamd.alloc_judge(S), ppamd.alloc_follow(S, n), ppamd.alloc_lane_change(S, n)
    st = ppamd.alloc_judge_stats(4, 8)
    bufs = (sc, tr, res, jd, fo, lc, st)
    before = [to_np(d) for d in bufs]

    def sweep(sets, n_sets=None, E=4, B=8, lcfg=True, lstate=True, jcfg=True, stats=True, n_frames=2, ecfg=None):
        arr = (ppamd.Params * len(sets))(*sets)
        cfg = ppamd.SweepCfg(len(sets) if n_sets is None else n_sets, 0, 1, 0, ppamd.RolloutCfg(n_frames, 3, 300.0),
                             ppamd.SummaryCfg(E, B, 0, 100.0, 0, 0))
        b, T, R = ppamd.scene_struct(sc), ppamd.traffic_struct(tr), ppamd.result_struct(res)
        J, F, L, O = ppamd.judge_struct(jd), ppamd.follow_struct(fo), ppamd.lane_change_struct(lc), ppamd.stats_struct(st)
        ref = C.byref
        return ppamd.lib.pp_rollout_sweep(
            m.handle, arr, ref(cfg), ref(ecfg or ppamd.default_episode_cfg()),
            ref(ppamd.default_judge_cfg()) if jcfg else None, ref(ppamd.default_follow_cfg()),
            ref(ppamd.default_lane_change_cfg()) if lcfg else None, ref(b), ref(T), ref(R), ref(J), ref(F),
            ref(L) if lstate else None, ref(O) if stats else None, 0, None)

    assert sweep([good], n_sets=0) == -1 and sweep([good], n_sets=-2) == -1
    assert sweep([good, ppamd.default_params(n_speeds=9)]) == -1
    assert sweep([good, ppamd.default_params(n_draws=4)]) == -1
    assert sweep([good, ppamd.default_params(emit_paths=True)]) == -1
    assert sweep([good], lcfg=False) == -1 and sweep([good], lstate=False) == -1
    assert sweep([good], jcfg=False) == -1 and sweep([good], stats=False) == -1
    assert sweep([good], E=0) == -1 and sweep([good], B=0) == -1 and sweep([good], n_frames=-1) == -1
    assert sweep([good], ecfg=ppamd.default_episode_cfg(n_cars=13)) == -1       # beyond the buffers' 12 cars
    for d, was in zip(bufs, before):
        same_bits(was, to_np(d), "buffers")


@pytest.mark.parametrize("B,hist_max", [(64, 2000.0), (1024, 1999.0), (7, 3000.0)])
def test_stats_quantile(B, hist_max):
    S = 65537
    j = random_state(S)
    st = host_summary(j, S, 30000, B=B, hist_max=hist_max)
    for row in range(3):
        sl = slice(row * 30000, min(S, (row + 1) * 30000))
        ok = (j["steps"][sl] != 0) & np.isfinite(j["dist"][sl]) & np.isfinite(j["clean_dist"][sl])
        x = np.sort(j["clean_dist"][sl][ok])
        for q in (0.1, 0.5, 0.9):
            lo, hi = ppamd.stats_quantile(st, row, q, hist_max)
            v = x[math.ceil(q * len(x)) - 1]
            assert lo <= v < hi, (row, q, lo, v, hi)
            assert hi - lo <= hist_max / B * (1 + 1e-12) or hi == INF
    assert all(math.isnan(e) for e in ppamd.stats_quantile(ppamd.alloc_judge_stats(1, 4), 0, 0.5, 4.0))


# ---- GPU ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
class TestJudgeSummaryGPU:
    @pytest.fixture(scope="class")
    def env(self):
        import torch
        wx, wy = oracle_lib.highway_map()
        return {"m": ppamd.Map(wx, wy), "torch": torch, "dev": torch.device("cuda", 0)}

    def device_summary(self, env, jd, S, E, B=64, hist_max=2000.0, **kw):
        st = ppamd.judge_summary(jd, S, E, hist_bins=B, hist_max=hist_max, m=env["m"], device=0, **kw)
        env["torch"].cuda.synchronize()
        return to_np(st)

    def upload(self, env, j):
        t = env["torch"]
        return {k: t.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(env["dev"]) for k, v in j.items()}

    @pytest.mark.parametrize("S", SIZES)
    def test_device_equals_host_bits(self, env, S):
        """Every stats array: one scene, either side of the tile edge, several tiles, 257 tiles (the
        group kernel's lane 0 takes two); groups below a tile and of exactly one (rows written by the
        tile kernel itself), of several tiles, short last groups, and the whole state; the state
        untouched; a second call the same bits."""
        j = random_state(S)
        jd = self.upload(env, j)
        for E in (1, 100, 256, 1000, S):
            if E == 1 and S > 1000:
                continue
            for B, hist_max in ((1, 5.0), (64, 2000.0), (1024, 1999.0)):
                got = self.device_summary(env, jd, S, E, B, hist_max)
                same_bits(host_summary(j, S, E, B, hist_max), got, f"S={S} E={E} B={B}")
        again = self.device_summary(env, jd, S, E, B, hist_max)
        same_bits(got, again, "second call")
        same_bits(j, ppamd.judge_to_numpy(jd), "state")

    def test_chunks_of_several_tiles(self, env):
        """Above 1,024 tiles a block takes a chunk of consecutive tiles of its group (4 at this size).
        599,291 scenes are 2,341 tiles, an odd count: as one group, the last chunk holds one tile; as
        groups of 200,000 (782 tiles, 196 chunks) the last chunk of each holds two, and the short third
        group leaves a whole chunk empty; groups of 100,000 (391 tiles) end in a chunk of three. The
        velocity rings, which the summary never reads, stay zero on both sides and are not uploaded."""
        S = 599291
        j = random_state(S)
        t, dev = env["torch"], env["dev"]
        jd = {k: (t.zeros(v.shape, dtype=t.float64, device=dev) if k.startswith("ring_") else
                  t.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev)) for k, v in j.items()}
        for E in (S, 200000, 100000):
            got = self.device_summary(env, jd, S, E, 64, 2000.0)
            same_bits(host_summary(j, S, E, 64, 2000.0), got, f"E={E}")
        same_bits(got, self.device_summary(env, jd, S, E, 64, 2000.0), "second call")
        small = {k: v for k, v in j.items() if not k.startswith("ring_")}
        same_bits(small, {k: v for k, v in ppamd.judge_to_numpy({k: jd[k] for k in small}).items()}, "state")
        o = oracle(j, S, S, 64, 2000.0)
        check_against_oracle(got if E == S else self.device_summary(env, jd, S, S, 64, 2000.0), o, "599,291 scenes")

    def test_out_rows_on_device(self, env):
        S, E, B, R, first = 1000, 300, 16, 9, 2
        j = random_state(S)
        jd = self.upload(env, j)
        std = ppamd.alloc_judge_stats(R, B, xp="torch", device=env["dev"])
        sth = ppamd.alloc_judge_stats(R, B)
        for d in (std, sth):
            for v in d.values():
                v[...] = 77
        self.device_summary(env, jd, S, E, B, stats=std, out_first=first)
        host_summary(j, S, E, B, stats=sth, out_first=first)
        same_bits(sth, to_np(std), "rows")

    def drive(self, env, S, F, prm, seed=31):
        t, dev, m = env["torch"], env["dev"], env["m"]
        judge, follow = ppamd.alloc_judge(S, xp="torch", device=dev), ppamd.alloc_follow(S, 12, xp="torch", device=dev)
        lc = ppamd.alloc_lane_change(S, 12, xp="torch", device=dev)
        d, g = ppamd.synth_episode(m, S, seed=seed, device=0, judge=judge, follow=follow)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        ppamd.rollout_lane_changing(m, d, g, prm, res, follow, lc, F, 3, 300.0, judge=judge)
        return judge

    def test_after_a_real_rollout(self, env):
        """1000 scenes x 40 frames of lane-changing traffic from pp_synth_episode."""
        S = 1000
        jd = self.drive(env, S, 40, ppamd.default_params())
        env["torch"].cuda.synchronize()
        j = ppamd.judge_to_numpy(jd)
        assert (j["steps"] == ppamd.JUDGE_RING + 120).all() and j["dist"].max() > 10
        for E in (100, 256, S):
            got = self.device_summary(env, jd, S, E, 64, 80.0)
            same_bits(host_summary(j, S, E, 64, 80.0), got, f"E={E}")
            check_against_oracle(got, oracle(j, S, E, 64, 80.0), f"rollout E={E}")
            same_bits(got, self.device_summary(env, jd, S, E, 64, 80.0), "second call")
        same_bits(j, ppamd.judge_to_numpy(jd), "state")

    def test_sweep_equals_the_calls_made_by_hand(self, env):
        """Three sets (defaults; keep_distance 30; comfort cost mode with n_speeds 3) and the first one
        again, 1024 scenes in G = 2 groups of 512, 30 frames: every row equals the by-hand sequence bit for
        bit, and the repeated set's rows equal the first's."""
        S, E, F, B, hm = 1024, 512, 30, 64, 64.0
        kd30 = ppamd.default_params()
        kd30.keep_distance = 30.0
        sets = [ppamd.default_params(), kd30, ppamd.default_params(n_speeds=3, cost_mode=ppamd.COST_COMFORT),
                ppamd.default_params()]
        stats, buf = ppamd.rollout_sweep(env["m"], sets, S, F, scenes_per_group=E, seed=31, hist_bins=B, hist_max=hm)
        env["torch"].cuda.synchronize()
        stats = to_np(stats)
        G = 2
        assert stats["n_scenes"].tolist() == [E] * (len(sets) * G)
        rows = lambda p: {k: v[..., p * G:(p + 1) * G] for k, v in stats.items()}
        for p, prm in enumerate(sets[:3]):
            hand = self.device_summary(env, self.drive(env, S, F, prm), S, E, B, hm)
            same_bits(hand, rows(p), f"set {p}")
            assert hand["n_unjudged"].sum() == 0 and hand["steps"].tolist() == [E * (ppamd.JUDGE_RING + 3 * F)] * G
        same_bits(rows(0), rows(3), "repeated set")
        differ = [k for k in ("dist_sum", "clean_dist_sum") if not np.array_equal(rows(0)[k], rows(1)[k])]
        assert differ, "keep_distance 30 drove exactly as keep_distance 10: the sets did not reach the planner"
        # the buffers handed back drive again: the same rows
        stats2, _ = ppamd.rollout_sweep(env["m"], sets[:1], S, F, scenes_per_group=E, seed=31, hist_bins=B,
                                        hist_max=hm, buffers=buf)
        env["torch"].cuda.synchronize()
        same_bits(rows(0), to_np(stats2), "reused buffers")
