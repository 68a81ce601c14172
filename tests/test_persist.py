"""The persistent K2 of reference mode (pp_eval, include/pp.h PP_DBG_PERSIST): k_cand<Persist, 1>
runs as many blocks as the device holds at once; block b takes group b and then the groups it
claims from a counter of the stream's workspace, which pp_eval zeroes on the stream ahead of K1.
The groups are cand_group's own, so every output must equal the one-group-per-block launch's BIT
FOR BIT: winner, n_out, next_x/y, cost, status, with the scenes k_prep routes to k_cand<true>
among them. R is the resident block count the library reports (PP_DBG_LAST_PERSIST); the batch
sizes put fewer groups than blocks, a few more than blocks with a partial last group, and more
than two claims per block around it."""
import threading

import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from slow_route_lib import speed_edge_scenes

pytestmark = pytest.mark.gpu
SPB = 17                        # scenes per k_cand group at the default 15 candidates


@pytest.fixture(scope="module")
def env():
    import torch
    wx, wy = oracle_lib.highway_map()
    e = {"torch": torch, "m": ppamd.Map(wx, wy), "wx": wx, "wy": wy,
         "olib": oracle_lib.load_oracle(), "dev": torch.device("cuda", 0)}
    # R: the persistent K2's resident blocks, from a first (3-group) call
    run(e, to_dev(e, ppamd.synth_host(e["m"], 3 * SPB, seed=1, first=1)), ppamd.default_params(), ppamd.PERSIST_ON)
    e["R"] = ppamd.debug_get(ppamd.DBG_LAST_PERSIST)
    assert e["R"] >= 1
    return e


def to_dev(env, sc):
    return {k: env["torch"].from_numpy(np.ascontiguousarray(v)).to(env["dev"]) for k, v in sc.items()}


def run(env, d, prm, persist, stream=None, sync=True):
    """One evaluation in the three-kernel shape on one stream (small batches would otherwise run the
    fused step, shard-sized ones the multi-stream split), the persistent K2 forced on or off."""
    S = int(d["ego_x"].shape[0])
    r = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
    with ppamd.debug(ppamd.DBG_SHAPE, ppamd.SHAPE_SPLIT), ppamd.debug(ppamd.DBG_SPLIT, ppamd.SPLIT_OFF), \
            ppamd.debug(ppamd.DBG_PERSIST, persist):
        if stream is None:
            ppamd.evaluate(env["m"], d, prm, r, device=0)
        else:
            ppamd.evaluate(env["m"], d, prm, r, device=0, stream=stream.cuda_stream)
    if sync:
        env["torch"].cuda.synchronize()
        return ppamd.result_to_numpy(r)
    return r


def assert_same_bits(a, b):
    for k in ("winner", "n_out", "next_x", "next_y", "cost", "status"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), k


def on_off(env, sc, prm=None):
    """The batch with the persistent K2 and without it; the two results, bit-identical."""
    prm = prm or ppamd.default_params()
    d = to_dev(env, sc)
    a = run(env, d, prm, ppamd.PERSIST_ON)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == env["R"]      # the persistent kernel really ran
    b = run(env, d, prm, ppamd.PERSIST_OFF)
    assert ppamd.debug_get(ppamd.DBG_LAST_PERSIST) == 0
    assert_same_bits(a, b)
    return a, b


def test_three_groups_vs_oracle(env):
    """51 scenes = 3 groups: all blocks but three draw no group and leave; the result also equals
    the oracle (oracle_lib.compare)."""
    sc = ppamd.synth_host(env["m"], 3 * SPB, seed=51, first=51)
    prm = ppamd.default_params()
    a, _ = on_off(env, sc, prm)
    ref = oracle_lib.oracle_eval(env["olib"], env["wx"], env["wy"], sc, prm, info=False)
    oracle_lib.compare(a, ref)


@pytest.mark.parametrize("shape", ["R+5_partial", "2R+1"])
def test_claimed_groups_bit_identical(env, shape):
    """R + 5 groups and 3 scenes more (five blocks claim a second group, the last group is partial),
    and 2 R + 1 groups (every block's claims go past the batch's end at different times)."""
    R = env["R"]
    S = (R + 5) * SPB + 3 if shape == "R+5_partial" else (2 * R + 1) * SPB
    on_off(env, ppamd.synth_host(env["m"], S, seed=S, first=S))


def test_flagged_and_frame0_scenes_bit_identical(env):
    """Frame-0 scenes and scenes k_prep flags kLimSlow among the fast ones, over more groups than
    blocks: the persistent kernel skips the flagged scenes of a group exactly as k_cand<false>
    does, and k_cand<true> runs them after it from the same list."""
    S = (env["R"] + 40) * SPB + 5
    a, _ = on_off(env, speed_edge_scenes(env["m"], S))
    assert (a["status"] != 0).any()


def test_two_calls_back_to_back_reset_the_counter(env):
    """Two calls of different sizes on one stream without a host synchronisation between them: the
    second call's claims start from zero again (the counter is reset on the stream), whichever
    value the first left in it."""
    R, prm = env["R"], ppamd.default_params()
    S1, S2 = (2 * R + 7) * SPB + 1, (R + 3) * SPB + 9
    d1 = to_dev(env, ppamd.synth_host(env["m"], S1, seed=11, first=S1))
    d2 = to_dev(env, ppamd.synth_host(env["m"], S2, seed=12, first=S2))
    r1 = run(env, d1, prm, ppamd.PERSIST_ON, sync=False)
    r2 = run(env, d2, prm, ppamd.PERSIST_ON, sync=False)
    r3 = run(env, d1, prm, ppamd.PERSIST_ON, sync=False)
    env["torch"].cuda.synchronize()
    a1, a2, a3 = (ppamd.result_to_numpy(r) for r in (r1, r2, r3))
    assert_same_bits(a1, run(env, d1, prm, ppamd.PERSIST_OFF))
    assert_same_bits(a2, run(env, d2, prm, ppamd.PERSIST_OFF))
    assert_same_bits(a3, a1)


def test_two_streams_at_once(env):
    """Two callers on their own streams at the same time: each stream's workspace has its own
    counter, so neither call takes or loses a group of the other."""
    torch, R, prm = env["torch"], env["R"], ppamd.default_params()
    sizes = [(2 * R + 3) * SPB + 2, (R + 9) * SPB]
    ds = [to_dev(env, ppamd.synth_host(env["m"], S, seed=100 + i, first=S)) for i, S in enumerate(sizes)]
    want = [run(env, d, prm, ppamd.PERSIST_OFF) for d in ds]
    got, errors = [None, None], []

    def worker(i):
        try:
            st = torch.cuda.Stream(env["dev"])
            for _ in range(3):
                r = ppamd.alloc_result(sizes[i], prm, xp="torch", device=env["dev"])
                ppamd.evaluate(env["m"], ds[i], prm, r, device=0, stream=st.cuda_stream)
                st.synchronize()
                got[i] = ppamd.result_to_numpy(r)
                assert_same_bits(got[i], want[i])
        except BaseException as ex:                # reported by the main thread
            errors.append(f"caller {i}: {type(ex).__name__}: {ex}")

    with ppamd.debug(ppamd.DBG_SHAPE, ppamd.SHAPE_SPLIT), ppamd.debug(ppamd.DBG_SPLIT, ppamd.SPLIT_OFF), \
            ppamd.debug(ppamd.DBG_PERSIST, ppamd.PERSIST_ON):
        threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a caller did not finish"
    assert not errors, errors
    assert got[0] is not None and got[1] is not None
