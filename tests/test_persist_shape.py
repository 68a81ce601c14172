"""The persistent K2 with BASELINE config 5's shape as compile-time constants (k_cand<PersistShape, 1>,
cand_group's kShape: 5 speeds, 3 lanes, 17 scenes and 51 slots per group, teams of 5, no draws;
taken at config 5's horizon of 50 points).
pp_eval picks it when the call's geometry equals those constants and reports it through
PP_DBG_LAST_PERSIST_SHAPE; every other shape keeps the generic persistent kernel. Only integer
index arithmetic, loop bounds and LDS pointer arithmetic differ, so every output must equal the
one-group-per-block launch's (PERSIST_OFF, the untouched k_cand<false, 1>) BIT FOR BIT: winner,
n_out, next_x/y, cost, status. R is the persistent K2's resident block count."""
import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from slow_route_lib import speed_edge_scenes
from test_persist import SPB, assert_same_bits, run, to_dev

pytestmark = pytest.mark.gpu
OFFS8 = [-6, -4, -3, -2, -1, 0, 2]      # bench.py's offsets at n_speeds = 8


@pytest.fixture(scope="module")
def env():
    import torch
    wx, wy = oracle_lib.highway_map()
    e = {"torch": torch, "m": ppamd.Map(wx, wy), "wx": wx, "wy": wy,
         "olib": oracle_lib.load_oracle(), "dev": torch.device("cuda", 0)}
    run(e, to_dev(e, ppamd.synth_host(e["m"], 3 * SPB, seed=1, first=1)), ppamd.default_params(), ppamd.PERSIST_ON)
    e["R"] = ppamd.debug_get(ppamd.DBG_LAST_PERSIST)
    assert e["R"] >= 1
    return e


def on_off(env, sc, prm=None, shape=1):
    """The batch with the persistent K2 and without it, bit-identical; `shape`: whether the
    persistent call must have taken the shape-specialised instantiation."""
    prm = prm or ppamd.default_params()
    d = to_dev(env, sc)
    a = run(env, d, prm, ppamd.PERSIST_ON)
    # (R is the resident block count of config 5's 256-thread blocks; other geometries have their own)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == env["R"] if shape else ppamd.debug_get(ppamd.DBG_LAST_PERSIST) >= 1
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST_SHAPE) == shape
    b = run(env, d, prm, ppamd.PERSIST_OFF)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == 0 and ppamd.debug_get(ppamd.DBG_LAST_PERSIST_SHAPE) == 0
    assert_same_bits(a, b)
    return a


def test_three_groups_vs_oracle(env):
    """51 scenes = 3 groups; the result also equals the oracle (oracle_lib.compare)."""
    sc = ppamd.synth_host(env["m"], 3 * SPB, seed=51, first=51)
    prm = ppamd.default_params()
    a = on_off(env, sc, prm)
    oracle_lib.compare(a, oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, prm, info=False))


@pytest.mark.parametrize("shape", ["R+1scene", "R+5_partial", "2R+1"])
def test_claimed_groups_bit_identical(env, shape):
    """R groups and one scene (the last group holds one scene), R + 5 groups and 3 scenes, and
    2 R + 1 whole groups."""
    R = env["R"]
    S = {"R+1scene": R * SPB + 1, "R+5_partial": (R + 5) * SPB + 3, "2R+1": (2 * R + 1) * SPB}[shape]
    on_off(env, ppamd.synth_host(env["m"], S, seed=S, first=S))


def test_flagged_groups_between_fast_ones(env):
    S = (env["R"] + 40) * SPB + 5
    a = on_off(env, speed_edge_scenes(env["m"], S))
    assert (a["status"] != 0).any()


def mixed_scenes(m, S, seed=606):
    """n_prev 0, 1, 2 and 10 in turn; every fifth ego (its kept points with it) 25 m to the side of
    where the generator put it, off the road, so its candidates take the fallback spline; every
    seventh scene with one car, every eleventh with none."""
    sc = ppamd.synth_host(m, S, seed=seed, first=seed)
    sc["n_prev"][:] = np.array([0, 1, 2, 10], np.int32)[np.arange(S) % 4]
    hx, hy = sc["prev_x"][9] - sc["prev_x"][8], sc["prev_y"][9] - sc["prev_y"][8]
    nrm = np.maximum(np.hypot(hx, hy), 1e-12)
    off = np.where(np.arange(S) % 5 == 0, 25.0, 0.0)
    dx, dy = hy / nrm * off, -hx / nrm * off
    for k, dd in (("x", dx), ("y", dy)):
        sc["ego_" + k] += dd
        sc["prev_" + k] += dd[None, :]
    sc["n_cars"][np.arange(S) % 7 == 0] = 1
    sc["n_cars"][np.arange(S) % 11 == 0] = 0
    return sc


def test_mixed_batch_bit_identical(env):
    S = (env["R"] + 3) * SPB + 2
    sc = mixed_scenes(env["m"], S)
    a = on_off(env, sc)
    assert (a["status"] & 4).any()              # PP_ST_FALLBACK: the off-road egos' fallback spline


@pytest.mark.parametrize("case", ["n_speeds=4", "n_speeds=8", "n_points=30"])
def test_other_shapes_keep_the_generic_kernel(env, case):
    """Shapes that are not config 5's (its horizon of 50 points included) take the generic
    persistent kernel."""
    prm = {"n_speeds=4": ppamd.default_params(n_speeds=4),
           "n_speeds=8": ppamd.default_params(n_speeds=8, speed_offsets=OFFS8),
           "n_points=30": ppamd.default_params(n_points=30)}[case]
    C = ppamd.NUM_LANES * prm.n_speeds
    spb = {12: 16, 24: 8, 15: 17}[C]           # scenes per group (pp_launch.h cands_per_block)
    S = (2 * env["R"] + 5) * spb + 3            # more groups than any geometry's resident blocks
    on_off(env, ppamd.synth_host(env["m"], S, seed=S, first=S), prm, shape=0)
