"""What lane-changing traffic costs per frame (DESIGN.md "Lane-changing traffic"): pp_rollout_reactive
(judge on) against pp_rollout_lane_changing (judge on) on one GPU at 262,144 and 2,097,152 scenes, 12
cars, consume 3, from pp_synth_episode's start; and plain pp_rollout and pp_rollout_reactive alone,
for the comparison with a parent commit's library.

Every repetition starts each variant from the same episode start (one seed), runs 3 warm-up frames,
then times 20 frames between two events on the launch stream; the variants alternate and the median
of the repetitions is reported as ms per frame, with the difference (what k_lane_change adds), the
share of scenes and cars that began a change in the 23 frames, the bytes and operations
k_lane_change needs per scene counted from csrc/pp_lanechange.h (lane_change_counts below) and the
rate that makes. Writes profiles/lane_change_cost.json, stamped with the SHA-256 of the library
measured.

    python tools/lane_change_cost.py                # this build, both sizes
    python tools/lane_change_cost.py --lib OTHER.so --plain-only --out parent.json
                                                    # pp_rollout and pp_rollout_reactive of another build
                                                    # (a parent commit's library has no lane changes)
A run without a GPU fails; nothing here is an estimate."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "carnd-path-planning-project_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import ppamd  # noqa: E402  (structs and allocators; the library under test is opened below)
from follow_cost import open_lib as open_follow_lib  # noqa: E402

K_BLOCK = 2      # csrc/pp_lanechange.h kBlock
IDM = {"flops": 13, "div": 3}     # pplanechange::idm with a leader


def lane_change_counts(n_cars, lanes):
    """What k_lane_change needs per scene and frame in steady state with every car eligible
    (csrc/pp_lanechange.h). Bytes: each address of the batch arrays counted once per frame (the
    passes' re-reads come from cache). cache_bytes: those re-reads, the scan's among them. gathers:
    reads of the map's lane and arc tables at a per-scene index. flops/div/sqrt: FP64 operations."""
    n = n_cars
    slots = 2 * n * (lanes - 1) // lanes                          # directions inside the road, lanes equally used
    blocks = -(-n // K_BLOCK)
    read = 3 * 8 + 3 * 4 + n * (4 + 4 + 8 + 8 + 8) + n * (8 + 4 + 8) + n * (8 + 4)   # ego; started x2, ego_seg; traffic; follow records; home, wait
    write = 2 * 4 + n * (8 + 4 + 8 + 8 + 4)                       # last_car, last_dir; offset, wait, arc, gain, dir
    cache = n * (4 + 4 + 8 + 8 + 8 + 8 + 4 + 8 + 4 + 8 + 8) + blocks * n * (4 + 4 + 8)   # block set-up (+ the leader's speed); the scan
    proj = 5 * lanes                                              # the ego: hint +- 2 on every lane
    idms = n + 2 * n // 2 + 3 * slots                             # a_j; the old follower's two (about every other car has one); a_j', a_f', a_f
    return {"read": read, "write": write, "cache_bytes": cache,
            "gathers": proj * 4 + lanes * 2 + n * 2 + slots * (3 * 4 + 2 + 2 + 1),
            "flops": proj * 21 + lanes * 3 + n * 8 + slots * (3 * 21 + 3 + 8 + 12) + 2 * n * n * 4 + idms * IDM["flops"],
            "div": proj + 1 + 3 * slots + idms * IDM["div"], "sqrt": lanes + 1}


def open_lib(path):
    lib = open_follow_lib(path)
    lib.pp_synth_episode.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(ppamd.EpisodeCfg),
                                     C.POINTER(ppamd.FollowCfg), C.POINTER(ppamd.SceneBatch), C.POINTER(ppamd.Traffic),
                                     C.POINTER(ppamd.Judge), C.POINTER(ppamd.Follow), C.c_int32, C.c_void_p]
    lib.pp_episode_cfg_default.argtypes = [C.POINTER(ppamd.EpisodeCfg)]
    lib.pp_episode_cfg_default.restype = None
    if hasattr(lib, "pp_rollout_lane_changing"):
        lib.pp_rollout_lane_changing.argtypes = lib.pp_rollout_reactive.argtypes + [C.POINTER(ppamd.LaneChangeCfg),
                                                                                   C.POINTER(ppamd.LaneChange)]
        lib.pp_lane_change_cfg_default.argtypes = [C.POINTER(ppamd.LaneChangeCfg)]
        lib.pp_lane_change_cfg_default.restype = None
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=ppamd.LIB_PATH)
    ap.add_argument("--scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="pp_rollout and pp_rollout_reactive only")
    ap.add_argument("--out", help="default profiles/lane_change_cost.json; required with --lib or --plain-only")
    a = ap.parse_args()
    if a.out is None:
        if a.plain_only or os.path.abspath(a.lib) != os.path.abspath(ppamd.LIB_PATH):
            ap.error("--out is required with --lib or --plain-only (profiles/lane_change_cost.json is this build's record)")
        a.out = os.path.join(REPO, "profiles", "lane_change_cost.json")

    import torch
    assert torch.cuda.is_available(), "lane_change_cost.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lib = open_lib(a.lib)
    changing_ok = hasattr(lib, "pp_rollout_lane_changing") and not a.plain_only
    wx, wy = ppamd.highway_map()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert lib.pp_map_create(wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), len(wx), C.byref(h)) == 0
    prm = ppamd.Params()
    lib.pp_params_default(C.byref(prm))
    prm.n_speeds, prm.n_points = 1, 50
    jc, fc, ec, lc = ppamd.JudgeCfg(), ppamd.FollowCfg(), ppamd.EpisodeCfg(), ppamd.LaneChangeCfg()
    lib.pp_judge_cfg_default(C.byref(jc))
    lib.pp_follow_cfg_default(C.byref(fc))
    lib.pp_episode_cfg_default(C.byref(ec))
    if changing_ok:
        lib.pp_lane_change_cfg_default(C.byref(lc))
    n = ec.n_cars

    def one(S, variant):
        """ms per frame of one timed window from the seeded start; variant: plain, reactive, changing."""
        d = ppamd.add_car_table(ppamd.alloc_scenes(S, n, xp="torch", device=dev), xp="torch", device=dev)
        t = ppamd.alloc_traffic(S, n, xp="torch", device=dev)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        follow = ppamd.alloc_follow(S, n, xp="torch", device=dev)
        change = ppamd.alloc_lane_change(S, n, xp="torch", device=dev) if variant == "changing" else None
        b, T = ppamd.scene_struct(d), ppamd.traffic_struct(t)
        J, F = ppamd.judge_struct(judge), ppamd.follow_struct(follow)
        assert lib.pp_synth_episode(h, 20261020, 0, C.byref(ec), None, C.byref(b), C.byref(T), C.byref(J), C.byref(F),
                                    0, None) == 0
        R = ppamd.result_struct(res)
        L = ppamd.lane_change_struct(change) if change is not None else None

        def run(frames):
            cfg = ppamd.RolloutCfg(frames, a.consume, 300.0)
            args = (h, C.byref(b), C.byref(T), C.byref(prm), C.byref(cfg), C.byref(R), None, 0, None)
            if variant == "changing":
                rc = lib.pp_rollout_lane_changing(*args, C.byref(jc), C.byref(J), C.byref(fc), C.byref(F), C.byref(lc),
                                                  C.byref(L))
            elif variant == "reactive":
                rc = lib.pp_rollout_reactive(*args, C.byref(jc), C.byref(J), C.byref(fc), C.byref(F))
            else:
                rc = lib.pp_rollout(*args)
            assert rc == 0, rc

        run(a.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(a.frames)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.frames
        rec = None
        if variant != "plain":
            f = judge["flags"].cpu().numpy().view(np.uint32)
            rec = {k: int(((f >> i) & 1).sum()) for i, k in enumerate(ppamd.INC_KINDS)}
            rec["clean"] = int((f == 0).sum())
        if change is not None:
            rec["scenes_with_a_change"] = int((change["n_changes"] > 0).sum().item())
            rec["cars_that_changed"] = int((change["changes"] > 0).sum().item())
            rec["changes"] = int(change["n_changes"].sum().item())
            rec["scene_share"] = rec["scenes_with_a_change"] / S
            rec["car_share"] = rec["cars_that_changed"] / (S * n)
        return ms, rec

    out = {"what": "ms per closed-loop frame, events on the launch stream; median of reps, variants alternating",
           "lib": os.path.basename(a.lib), "lib_sha256": ppamd.lib_sha256(a.lib), "gpu": torch.cuda.get_device_name(0),
           "frames": a.frames, "warmup": a.warmup, "consume": a.consume, "cars": n, "reps": a.reps, "sizes": {}}
    variants = ["plain", "reactive"] + (["changing"] if changing_ok else [])
    for S in a.scenes:
        one(S, "plain")                                         # first touch of the size: workspace allocation
        ms = {v: [] for v in variants}
        rec = {}
        for _ in range(a.reps):
            for v in variants:
                m, rec[v] = one(S, v)
                ms[v].append(m)
        r = {"rollout_ms": statistics.median(ms["plain"]), "rollout_ms_all": ms["plain"],
             "rollout_reactive_ms": statistics.median(ms["reactive"]), "rollout_reactive_ms_all": ms["reactive"],
             "reactive_scenes_with_incident": rec["reactive"]}
        if changing_ok:
            cnt = lane_change_counts(n, ppamd.NUM_LANES)
            add = statistics.median(ms["changing"]) - statistics.median(ms["reactive"])
            r.update({"rollout_lane_changing_ms": statistics.median(ms["changing"]),
                      "rollout_lane_changing_ms_all": ms["changing"], "lane_change_ms": add,
                      "lane_change_counts_per_scene": cnt,
                      "lane_change_GBps": (cnt["read"] + cnt["write"]) * S / (add * 1e-3) / 1e9 if add > 0 else None,
                      "lane_change_GFLOPs": cnt["flops"] * S / (add * 1e-3) / 1e9 if add > 0 else None,
                      "lane_changing_record": rec["changing"]})
        out["sizes"][str(S)] = r
        print(S, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "sizes"}))


if __name__ == "__main__":
    main()
