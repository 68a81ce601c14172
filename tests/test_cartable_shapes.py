"""Car-table mode (pp_scene_batch::tab_*, the reference's cross-frame std::map<int, Car>,
src/main.cpp:1194, 1325-1350) in every K1 and every launch shape, with any slot ids.

- CPU: the restatement's table loop (oracle/pp_oracle.c) with sparse, negative, -1 and INT32_MIN
  slot ids and INT32_MAX padding is grounded in the reference itself: 12 closed-loop episodes, each
  beside its own reference session, form one oracle batch of 12 scenes whose table is a Python dict
  per scene laid out as csrc/pp_cartable.h describes; every frame must equal the session's exactly.
  Live where oracle/_ref is built, and from tests/golden/cartable_golden.npz everywhere.
- GPU: two consecutive frames of table state (cartable_lib.table_frames: an empty poisoned table,
  then the oracle's table after frame 1 with cars reported again, stale, erased and new) through
  the one-lane k_prep (3- and 4-wave builds), prep_grp_eval<2..16>, k_cand_small, the step kernel's
  three block shapes, the forced split, the persistent K2, a global-memory map, the K2 variants and
  pp_plan_batch_host on both sides of its mirror bound. Results and pp_scene_info against the oracle
  (oracle_lib.compare, compare_info), the whole table after the call against the oracle's, every
  other input unchanged.

The table's doubles are held BIT FOR BIT: tab_vx/tab_vy are copies of inputs, and tab_s, tab_d,
tab_vs, tab_vd come from the lane_match / project_speed whose ego results compare_info already holds
to the oracle's bits (INFO_BITS)."""
import os

import numpy as np
import pytest

import cartable_lib as ct
import oracle_lib
from oracle_lib import ppamd
from test_maps import loop_map

SEED = 10                       # a seed at which every shape below meets cartable_lib.assert_coverage
GOLDEN = os.path.join(oracle_lib.GOLDEN, "cartable_golden.npz")
TAB = ct.TAB_I + ct.TAB_F


# ---- CPU: the restatement's table loop against the reference ------------------------------------
def check_census(c):
    assert c["stale"] > 0 and c["erased"] > 0 and c["minus1"] > 0, c     # the episodes really do all three
    assert 30 <= c["union"] <= ct.EP_SLOTS, c


@pytest.mark.skipif(oracle_lib.load_ref_session() is None, reason="oracle/_ref not built (no reference here)")
def test_oracle_table_batch_vs_reference_sessions():
    wx, wy = oracle_lib.highway_map()
    rec = ct.record_episodes(ppamd.Map(wx, wy), wx, wy, oracle_lib.load_ref_session())
    check_census(ct.check_oracle_table_batch(oracle_lib.load_oracle(), wx, wy, rec))


def test_oracle_table_batch_vs_fixture():
    wx, wy = oracle_lib.highway_map()
    G = np.load(GOLDEN)
    check_census(ct.check_oracle_table_batch(oracle_lib.load_oracle(), wx, wy, {k: G[k] for k in G.files}))


def test_dict_layout_pads_and_takes_back():
    """The restated CarTable: union ascending, stored state or poison, INT32_MAX padding; take-back
    sets valid slots and erases invalid ones."""
    tab = ct.empty_table(5, 2)
    cars = {7: (1, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0), -1: (0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0)}
    assert ct.dict_layout(cars, [ct.I32_MIN, 7], tab, 1) == 3
    assert tab["tab_id"][:, 1].tolist() == [ct.I32_MIN, -1, 7, ct.I32_MAX, ct.I32_MAX]
    assert tab["tab_valid"][:, 1].tolist() == [0, 1, 1, 0, 0] and tab["tab_lane"][:, 1].tolist()[1:3] == [0, 1]
    assert np.isnan(tab["tab_s"][[0, 3, 4], 1]).all() and tab["tab_vy"][2, 1] == 6.0
    assert (tab["tab_id"][:, 0] == ct.I32_MAX).all()                      # the other scene: untouched
    tab["tab_valid"][:, 1] = [1, 0, 1, 0, 0]
    tab["tab_lane"][0, 1], tab["tab_s"][0, 1] = 2, 11.0
    ct.dict_take_back(cars, tab, 1, 3)
    assert sorted(cars) == [ct.I32_MIN, 7] and cars[ct.I32_MIN][:2] == (2, 11.0)


@pytest.mark.parametrize("S,K,ids", [(37, 1, True), (37, 17, True), (37, 33, False), (300, 5, True)])
def test_table_frames_contract(S, K, ids):
    """The generator keeps the batch contract (include/pp.h): rows ascending and distinct, every row
    id one of the slot ids, slot ids ascending with INT32_MAX padding, garbage beyond n_cars; and its
    coverage conditions hold on the CPU too."""
    wx, wy = oracle_lib.highway_map()
    frames = ct.table_frames(ppamd.Map(wx, wy), S, K, K, SEED, ids)
    for b in frames:
        assert b["tab_valid"].shape == (K, S) and b["car_id"].shape == (K, S)
        for s in range(S):
            n = b["n_cars"][s]
            row = b["car_id"][:n, s].astype(np.int64)
            assert (np.diff(row) > 0).all()
            slots = b["tab_id"][:, s] if ids else np.arange(K)
            assert (np.diff(slots.astype(np.int64)) >= 0).all() and np.isin(row, slots).all()
            assert np.isnan(b["car_x"][n:, s]).all() and np.isfinite(b["car_x"][:n, s]).all()
        assert not b["tab_valid"].any() and np.isnan(b["tab_s"]).all() and (b["tab_lane"] == ct.I32_MAX).all()
        if ids and K >= 5:
            assert 3 * (b["tab_id"] == -1).any(0).sum() >= S              # -1 in a third of the scenes at least
    ora = ct.oracle_frames(oracle_lib.load_oracle(), wx, wy, frames, ppamd.default_params())
    ct.assert_coverage(ct.coverage(ora), S, K, ids)


# ---- GPU: every K1 path in table mode against the oracle ----------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    e = {"torch": torch, "dev": torch.device("cuda", 0), "olib": oracle_lib.load_oracle(), "worlds": {}, "cases": {}}
    for name, (wx, wy) in (("highway", oracle_lib.highway_map()), ("loop2000", loop_map(2000))):
        e["worlds"][name] = (ppamd.Map(wx, wy), wx, wy)
    return e


def prm_key(prm):
    return (prm.n_speeds, prm.cost_mode, prm.emit_paths)


def table_case(env, world, S, K, ids, prm):
    """The two frames and the oracle's answers for them, computed once per shape and shared; the
    coverage conditions are asserted on what the oracle really did."""
    key = (world, S, K, ids) + prm_key(prm)
    if key not in env["cases"]:
        m, wx, wy = env["worlds"][world]
        frames = ct.table_frames(m, S, K, K, SEED, ids)
        ora = ct.oracle_frames(env["olib"], wx, wy, frames, prm)
        ct.assert_coverage(ct.coverage(ora), S, K, ids)
        for inp, res, table in ora:
            for d in (inp, res, table):
                for v in d.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
        env["cases"][key] = ora
    return env["cases"][key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_table(got, inp, want, what):
    """The table after a call against the oracle's: ids, valid and lane exact, the six double
    arrays bit for bit (poison NaNs included); a slot no row reported holds what it held, and so
    does an erased slot apart from its valid flag."""
    for k in TAB:
        if inp.get(k) is None:
            continue
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} slots, first (slot, scene) {np.argwhere(bad)[0]}"
    _, rep = ct.slot_view(inp)
    erased = rep & (got["tab_valid"] == 0)
    for k in TAB[1:]:
        keep = ~rep if k == "tab_valid" else ~rep | erased
        assert (bits(got[k])[keep] == bits(inp[k])[keep]).all(), (what, k)


def check_table_frames(env, world, case, prm, switches):
    """Both frames through pp_eval under the debug switches [(key, value)]: frame 1 from the empty
    poisoned table, frame 2 from the ORACLE's table after frame 1 (uploaded, so a frame-1
    discrepancy cannot cascade). Returns the read-only debug keys after frame 2."""
    t, m = env["torch"], env["worlds"][world][0]
    last = {}
    for f, (inp, ref, table) in enumerate(case):
        S = int(inp["ego_x"].shape[0])
        d = {k: t.from_numpy(np.array(v)).to(env["dev"]) for k, v in inp.items() if v is not None}
        d.update({k: None for k, v in inp.items() if v is None})
        r = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"], info=True)
        ctx = [ppamd.debug(k, v) for k, v in switches]
        for c in ctx:
            c.__enter__()
        try:
            ppamd.evaluate(m, d, prm, r, device=0)
            t.cuda.synchronize()
            last = {k: ppamd.debug_get(k) for k in (ppamd.DBG_LAST_PARTS, ppamd.DBG_LAST_PERSIST)}
        finally:
            for c in reversed(ctx):
                c.__exit__(None, None, None)
        got = ppamd.result_to_numpy(r)
        after = {k: v.cpu().numpy() for k, v in d.items() if v is not None}
        oracle_lib.compare(got, ref)
        oracle_lib.compare_info(got["info"], ref["info"])
        check_table(after, inp, table, f"frame {f + 1}")
        for k, v in inp.items():
            if v is not None and k not in TAB:
                assert (bits(after[k]) == bits(v)).all(), f"frame {f + 1}: input {k} was written"
    return last


SPLIT_SHAPE = (ppamd.DBG_SHAPE, ppamd.SHAPE_SPLIT)
ONE_LANE = [((ppamd.DBG_PREP_GROUP, 1), SPLIT_SHAPE, (ppamd.DBG_PREP_WAVES, w)) for w in (3, 4)]


@pytest.mark.gpu
class TestTableShapesGPU:
    @pytest.mark.parametrize("waves", [3, 4])
    @pytest.mark.parametrize("S,K", [(S, K) for S in (37, 300) for K in (1, 5, 17, 33)] + [(64, ppamd.MAX_CARS)])
    def test_one_lane_k_prep(self, env, S, K, waves):
        """k_prep's merge pointer over the ascending rows, 3- and 4-wave builds."""
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", S, K, True, prm), prm, ONE_LANE[waves - 3])

    @pytest.mark.parametrize("G", [2, 4, 8, 16])
    @pytest.mark.parametrize("S,K", [(S, K) for S in (37, 300) for K in (1, 5, 17, 33)])
    def test_grouped_k_prep(self, env, S, K, G):
        """prep_grp_eval<G>: the `ncar <= G` shortcut (K = 1, 5 and the scenes of few rows), the
        multi-round row scan (up to 33 rows), padding slots, partial groups in the last wave (S = 37)."""
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", S, K, True, prm), prm,
                           [(ppamd.DBG_PREP_GROUP, G), SPLIT_SHAPE])

    def test_cand_small(self, env):
        """the grouped K1 ahead of the fused K2/K4 launch"""
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", 300, 17, True, prm), prm,
                           [(ppamd.DBG_SHAPE, ppamd.SHAPE_CAND_SMALL)])

    @pytest.mark.parametrize("S", [9, 2049, 4097])
    def test_step_kernel(self, env, S):
        """prep_grp_eval<16> inside the one-launch step: 8-scene blocks of 256 threads, 16-scene
        blocks of 512 (k_step_small512), 16-scene blocks of 256; every scene is compared."""
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", S, 17, True, prm), prm,
                           [(ppamd.DBG_SHAPE, ppamd.SHAPE_STEP)])

    @pytest.mark.parametrize("K", [17, 33])
    def test_automatic_choice(self, env, K):
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", 300, K, True, prm), prm, [])

    def test_forced_split(self, env):
        """two parts, each K1 -> K2 -> K4 on its own stream, over one table"""
        prm = ppamd.default_params()
        last = check_table_frames(env, "highway", table_case(env, "highway", 2500, 17, True, prm), prm,
                                  [(ppamd.DBG_SPLIT, ppamd.SPLIT_ON), (ppamd.DBG_PREP_GROUP, 1), SPLIT_SHAPE])
        assert last[ppamd.DBG_LAST_PARTS] == 2                     # the split really ran

    def test_persistent_k2(self, env):
        prm = ppamd.default_params()
        last = check_table_frames(env, "highway", table_case(env, "highway", 300, 17, True, prm), prm,
                                  [(ppamd.DBG_PERSIST, ppamd.PERSIST_ON), (ppamd.DBG_SPLIT, ppamd.SPLIT_OFF), SPLIT_SHAPE])
        assert last[ppamd.DBG_LAST_PERSIST] >= 1                   # the persistent kernel really ran

    @pytest.mark.parametrize("group", [1, 0])
    def test_global_memory_map(self, env, group):
        """2,000 waypoints: the map is read from global memory (one-lane and grouped K1)"""
        prm = ppamd.default_params()
        check_table_frames(env, "loop2000", table_case(env, "loop2000", 300, 17, True, prm), prm,
                           [(ppamd.DBG_PREP_GROUP, group)] + ([SPLIT_SHAPE] if group == 1 else []))

    @pytest.mark.parametrize("variant", ["comfort", "paths"])
    def test_k2_variants_over_a_table(self, env, variant):
        """K1 is the same kernel; the K2s behind it read the prep record a table frame left"""
        prm = (ppamd.default_params(cost_mode=ppamd.COST_COMFORT) if variant == "comfort"
               else ppamd.default_params(emit_paths=True))
        check_table_frames(env, "highway", table_case(env, "highway", 300, 17, True, prm), prm, [])

    @pytest.mark.parametrize("path,S,switches", [
        ("one_lane", 300, ONE_LANE[0]), ("g4", 37, [(ppamd.DBG_PREP_GROUP, 4), SPLIT_SHAPE]),
        ("step", 9, [(ppamd.DBG_SHAPE, ppamd.SHAPE_STEP)])])
    def test_without_tab_id(self, env, path, S, switches):
        """tab_id NULL: slot k is id k"""
        prm = ppamd.default_params()
        check_table_frames(env, "highway", table_case(env, "highway", S, 17, False, prm), prm, switches)

    @pytest.mark.parametrize("S", [512, 513])
    def test_plan_batch_host(self, env, S):
        """pp_plan_batch_host copies the table in and back: through its pinned mirror (S <= 512,
        kStageMirrorMax) and by one asynchronous copy per field (beyond), on host dicts."""
        prm = ppamd.default_params()
        m = env["worlds"]["highway"][0]
        for f, (inp, ref, table) in enumerate(table_case(env, "highway", S, 17, True, prm)):
            host = {k: (None if v is None else np.array(v)) for k, v in inp.items()}
            got = ppamd.plan_batch_host(m, host, prm)
            oracle_lib.compare(got, ref)
            check_table(host, inp, table, f"frame {f + 1}")
            assert np.array_equal(host["tab_id"], inp["tab_id"])
            for k, v in inp.items():
                if k not in TAB:
                    assert (bits(host[k]) == bits(v)).all(), k
