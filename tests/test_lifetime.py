"""What a map holds on a device comes back when it is closed, and a refused allocation leaves it usable.

Every device allocation, pinned allocation, stream and event of the library is held by an owning
type ("Ownership of device resources"); pp_map_destroy releases a device's state
while that device is current. These tests look at the device from outside: free memory across
create / use / close cycles, and the library's answers after pp_reserve was refused."""
import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd

pytestmark = pytest.mark.gpu

CYCLES = 12
S_BIG, ROWS = 65_536, 12
# One cycle's large buffers, per scene: the prep workspace (12 + 4 NL f64 + 7 i32),
# the winner record as allocated (3 x 128 f64 + 2 u64) and the sorted rows (36 B per row + 8)
PER_SCENE = ((12 + 4 * ppamd.NUM_LANES) * 8 + 7 * 4) + (3 * ppamd.MAX_POINTS + 2) * 8 + (36 * ROWS + 8)
LARGE = S_BIG * PER_SCENE              # 245.6 MB at three lanes


@pytest.fixture(scope="module")
def env():
    import torch
    wx, wy = oracle_lib.highway_map()
    dev = torch.device("cuda", 0)
    m = ppamd.Map(wx, wy)
    big = ppamd.synth_device(m, S_BIG, seed=0x11FE, device=0, car_stride=ROWS)
    small = ppamd.synth_device(m, 2048, seed=0x11FF, device=0)
    host = ppamd.synth_host(m, 64, seed=0x1200)
    torch.cuda.synchronize()
    m.close()
    return {"torch": torch, "wx": wx, "wy": wy, "dev": dev, "big": big, "small": small, "host": host,
            "side": torch.cuda.Stream(dev)}


def head(sc, n):
    return {k: v[..., :n].contiguous() for k, v in sc.items()}


def cycle(env, second_device=False):
    """One map's life: every kind of device resource the library makes, then Map.close()."""
    t, dev = env["torch"], env["dev"]
    ref = ppamd.default_params()
    m = ppamd.Map(env["wx"], env["wy"])
    # the large buffers, on a side stream: prep workspace, winner record, sorted rows (K0 runs ahead
    # of the one-lane K1 only; at exactly 65,536 scenes the library would pick two K1 lanes per scene)
    r = ppamd.alloc_result(S_BIG, ref, xp="torch", device=dev)
    t.cuda.synchronize()
    with ppamd.debug(ppamd.DBG_SORT_CARS, 1), ppamd.debug(ppamd.DBG_PREP_GROUP, 1):
        ppamd.evaluate(m, env["big"], ref, r, device=0, stream=env["side"].cuda_stream)
    env["side"].synchronize()
    used = t.cuda.mem_get_info(0)[0]
    # the null stream's workspace
    m.reserve(0, 4096)
    # the split's streams and events
    r2 = ppamd.alloc_result(2048, ref, xp="torch", device=dev)
    with ppamd.debug(ppamd.DBG_SPLIT, ppamd.SPLIT_ON), ppamd.debug(ppamd.DBG_PREP_GROUP, 1), \
            ppamd.debug(ppamd.DBG_SHAPE, ppamd.SHAPE_SPLIT):
        ppamd.evaluate(m, env["small"], ref, r2, device=0)
        assert ppamd.debug_get(ppamd.DBG_LAST_PARTS) == 2
    s64 = head(env["small"], 64)
    for prm in (ppamd.default_params(cost_mode=ppamd.COST_COMFORT), ppamd.default_params(emit_paths=True)):
        ppamd.evaluate(m, s64, prm, ppamd.alloc_result(64, prm, xp="torch", device=dev), device=0)
    # the frame scratch and its stream
    h = env["host"]
    nc, npv = int(h["n_cars"][0]), int(h["n_prev"][0])
    cars = [(int(h["car_id"][j, 0]), h["car_x"][j, 0], h["car_y"][j, 0], h["car_vx"][j, 0], h["car_vy"][j, 0])
            for j in range(nc)]
    nx, _, _ = ppamd.plan_frame(m, h["ego_x"][0], h["ego_y"][0], h["ego_yaw_deg"][0], h["ego_speed_mph"][0],
                                h["prev_x"][:npv, 0], h["prev_y"][:npv, 0], cars,
                                target_lane=int(h["prev_target_lane"][0]))
    assert len(nx) == 50
    # the staging pair
    ppamd.plan_batch_host(m, h, ref)
    # the event pool
    m.timing(0, True)
    ppamd.evaluate(m, s64, ref, ppamd.alloc_result(64, ref, xp="torch", device=dev), device=0)
    _, launches = m.read_timing(0)
    assert launches[1] == 1
    # arctab
    sc, tr = ppamd.synth_traffic(m, 64, seed=0x1201, device=0)
    ppamd.traffic_follow(m, sc, tr, ppamd.alloc_follow(64, 12, xp="torch", device=dev), device=0)
    if second_device:
        d1 = t.device("cuda", 1)
        s1 = {k: v.to(d1) for k, v in s64.items()}
        ppamd.evaluate(m, s1, ref, ppamd.alloc_result(64, ref, xp="torch", device=d1), device=1)
        t.cuda.synchronize(1)
        t.cuda.set_device(0)          # (the map is closed with device 0 current)
    t.cuda.synchronize()
    m.close()
    return used, t.cuda.mem_get_info(0)[0]


def test_closed_maps_give_their_memory_back(env):
    """12 cycles of create, use, Map.close() on the highway map: free device memory after the last
    is at most one cycle's large buffers (245.6 MB) below free memory after the first, whose end is
    the baseline because torch's own cache is warm by then. Leaking the large buffers every cycle
    would cost eleven times that. The reference-mode evaluation is 65,536 scenes of 12 car rows with
    DBG_SORT_CARS 1 and, so that the pre-pass runs at that size, DBG_PREP_GROUP 1.

    Measured on an MI355X: the commit before the owning types (hand-written frees) passes at this
    size, so it stays at 65,536. Its free memory fell by 92,274,688 B between the end of cycle 1 and
    the end of cycle 2 (torch's cache, not the library: the owning types give the same figure) and by
    0 B from cycle 2 to cycle 12. Before its close a cycle holds 247,463,936 B more than after it;
    the test asks for that too (at least the large buffers), so that a runtime which returned freed
    memory late could not let a leak pass unseen."""
    t = env["torch"]
    multi = t.cuda.device_count() > 1
    _, first = cycle(env)
    for k in range(1, CYCLES):
        used, last = cycle(env, second_device=multi and k == 1)
        print(f"cycle {k + 1}: free {last} B after close, {first - last} B below cycle 1, {last - used} B less before the close")
    print(f"large buffers {LARGE} B")
    assert last - used >= LARGE
    assert first - last <= LARGE


def test_refused_allocation_leaves_the_map_usable(env):
    """pp_reserve for 2^44 scenes (3.8 PB of prep workspace) is refused on the host: PPError with
    status -3 (PP_ERR_NOMEM), nothing launched. The next pp_eval of the same 64 scenes on the null
    stream returns PP_OK and the first evaluation's result bit for bit: the refusal leaves neither a
    dangling workspace nor its error in the runtime for the next call's launch check to find."""
    t, dev = env["torch"], env["dev"]
    prm = ppamd.default_params()
    s64 = head(env["small"], 64)
    m = ppamd.Map(env["wx"], env["wy"])
    try:
        a = ppamd.alloc_result(64, prm, xp="torch", device=dev)
        ppamd.evaluate(m, s64, prm, a, device=0)
        t.cuda.synchronize()
        a = ppamd.result_to_numpy(a)
        with pytest.raises(ppamd.PPError) as ex:
            m.reserve(0, 2 ** 44)
        assert str(ex.value).endswith("status -3"), ex.value
        b = ppamd.alloc_result(64, prm, xp="torch", device=dev)
        ppamd.evaluate(m, s64, prm, b, device=0)           # (raises unless pp_eval returns PP_OK)
        t.cuda.synchronize()
        b = ppamd.result_to_numpy(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    finally:
        m.close()
