"""Episode starts in the four-lane build. Run by tests/test_episode.py in a child process whose
environment selects carnd-path-planning-project_amd/ppamd/libppamd_l4.so (PPAMD_LIB): a process
loads one PP_NUM_LANES. The per-lane cursors are PP_NUM_LANES-element arrays behind unrolled select
loops: the ego and the cars must use all four lanes, lane 3's cars keep their gaps like the others',
and the first follow update brakes nobody hard (tests 2 to 4 of tests/test_episode.py at S = 200, on
this library's own four-lane pp_map_geometry)."""
import pytest

import oracle_lib
import test_episode as te
from oracle_lib import ppamd


@pytest.fixture(scope="module")
def env():
    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    return {"m": m, "geo": te.Geo(m.geometry())}


def check(env, start):
    assert ppamd.NUM_LANES == 4 and env["geo"].NL == 4
    geo, S = env["geo"], 200
    cfg, fcfg = ppamd.default_episode_cfg(), ppamd.default_follow_cfg()
    sc, tr, judge, follow = start(S, cfg)
    lane, own, t = te.check_invariants(geo, sc, tr, judge, cfg)
    assert (tr["lane"][:12] == 3).any() and (lane == 3).any()
    te.check_gaps(geo, sc, tr, own, t, cfg, te.fdict(fcfg))
    te.check_first_follow(env["m"], geo, sc, tr, own, t, lane, cfg, te.fdict(fcfg))
    te.check_states(geo, sc, judge, follow)
    return sc, tr, judge, follow


def test_four_lanes_host(env):
    check(env, lambda S, cfg: te.make(env["m"], S, cfg=cfg))


@pytest.mark.gpu
def test_four_lanes_device(env):
    import torch
    dev = torch.device("cuda", 0)

    def start(S, cfg):
        sc, tr, judge, follow = te.device_start(env["m"], S, cfg=cfg, dev=dev)
        return te.to_np(sc), te.to_np(tr), ppamd.judge_to_numpy(judge), ppamd.follow_to_numpy(follow)

    got = check(env, start)
    want = te.make(env["m"], 200)
    for a, b, what in zip(got, want, ("scenes", "traffic", "judge", "follow")):
        a = {k: v for k, v in a.items() if hasattr(v, "tobytes")}
        te.same_bits(a, {k: (ppamd.judge_to_numpy(b)[k] if what == "judge" else b[k]) for k in a}, what)
