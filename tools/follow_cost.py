"""What reactive traffic costs per frame (DESIGN.md "Reactive traffic"): pp_rollout_judged against
pp_rollout_reactive with the judge on, on one GPU at 262,144 and 2,097,152 scenes, 12 cars,
consume 3; and plain pp_rollout, for the comparison with a parent commit's library.

Every repetition starts each variant from the same synthetic start state (pp_synth_traffic, one
seed), runs 3 warm-up frames, then times 20 frames between two events on the launch stream; the
variants alternate and the median of the repetitions is reported as ms per frame, with the
difference (what k_follow adds), the bytes and operations k_follow needs per scene counted from
csrc/pp_follow.h (follow_counts below) and the rate that makes. Writes profiles/follow_cost.json,
stamped with the SHA-256 of the library measured.

    python tools/follow_cost.py                     # this build, both sizes
    python tools/follow_cost.py --lib OTHER.so --plain-only --out parent.json
                                                    # pp_rollout alone of another build (a parent
                                                    # commit's library has no reactive traffic)
A run without a GPU fails; nothing here is an estimate."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "carnd-path-planning-project_amd"))

import numpy as np  # noqa: E402
import ppamd  # noqa: E402  (structs and allocators; the library under test is opened below)


def follow_counts(n_cars, lanes):
    """What k_follow needs per scene and frame in steady state (csrc/pp_follow.h). Bytes: each address
    of the batch arrays counted once per frame (the passes' re-reads come from cache). cache_bytes:
    those re-reads, the pair loop's among them. gathers: reads of the map's lane and arc tables at a
    per-scene index. flops/div/sqrt: FP64 operations."""
    n = n_cars
    read = 3 * 8 + 2 * 4 + n * (4 + 4 + 8 + 8 + 8)              # ego x, y, speed; started, ego_seg; lane, seg, t, speed, desired
    write = 2 * 4 + n * (8 + 4 + 8 + 8)                          # started, ego_seg; next_speed, leader, gap, speed
    pairs = n * (n - 1)
    cache = n * n * 4 + pairs // lanes * 8 + n * (4 + 8 + 8 + 4 + 8 + 8 + 8)   # pair loop: lane, arc of same-lane cars; passes 2-4
    proj = 5 * lanes                                             # hint +- 2 on every lane
    return {"read": read, "write": write, "cache_bytes": cache,
            "gathers": proj * 4 + lanes * 2 + n * 2 + n,         # segment ends; arc of the ego; arc of a car; loop
            "flops": proj * 21 + lanes * 3 + n * 2 + pairs // lanes * 3 + n * 22,
            "div": proj + 1 + 3 * n, "sqrt": lanes + 1}


def open_lib(path):
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    lib.pp_map_create.argtypes = [dp, dp, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pp_synth_traffic.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(ppamd.SceneBatch),
                                     C.POINTER(ppamd.Traffic), C.c_int32, C.c_void_p]
    lib.pp_rollout.argtypes = [C.c_void_p, C.POINTER(ppamd.SceneBatch), C.POINTER(ppamd.Traffic),
                               C.POINTER(ppamd.Params), C.POINTER(ppamd.RolloutCfg), C.POINTER(ppamd.Result),
                               C.POINTER(ppamd.RolloutLog), C.c_int32, C.c_void_p]
    lib.pp_params_default.argtypes = [C.POINTER(ppamd.Params)]
    lib.pp_params_default.restype = None
    if hasattr(lib, "pp_rollout_reactive"):
        lib.pp_rollout_judged.argtypes = lib.pp_rollout.argtypes + [C.POINTER(ppamd.JudgeCfg), C.POINTER(ppamd.Judge)]
        lib.pp_rollout_reactive.argtypes = lib.pp_rollout_judged.argtypes + [C.POINTER(ppamd.FollowCfg),
                                                                             C.POINTER(ppamd.Follow)]
        lib.pp_judge_cfg_default.argtypes = [C.POINTER(ppamd.JudgeCfg)]
        lib.pp_judge_cfg_default.restype = None
        lib.pp_follow_cfg_default.argtypes = [C.POINTER(ppamd.FollowCfg)]
        lib.pp_follow_cfg_default.restype = None
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=ppamd.LIB_PATH)
    ap.add_argument("--scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", help="default profiles/follow_cost.json; required with --lib or --plain-only")
    a = ap.parse_args()
    if a.out is None:
        if a.plain_only or os.path.abspath(a.lib) != os.path.abspath(ppamd.LIB_PATH):
            ap.error("--out is required with --lib or --plain-only (profiles/follow_cost.json is this build's record)")
        a.out = os.path.join(REPO, "profiles", "follow_cost.json")

    import torch
    assert torch.cuda.is_available(), "follow_cost.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lib = open_lib(a.lib)
    reactive_ok = hasattr(lib, "pp_rollout_reactive") and not a.plain_only
    wx, wy = ppamd.highway_map()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert lib.pp_map_create(wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), len(wx), C.byref(h)) == 0
    prm = ppamd.Params()
    lib.pp_params_default(C.byref(prm))
    prm.n_speeds, prm.n_points = 1, 50
    jc, fc = ppamd.JudgeCfg(), ppamd.FollowCfg()
    if reactive_ok:
        lib.pp_judge_cfg_default(C.byref(jc))
        lib.pp_follow_cfg_default(C.byref(fc))

    def one(S, variant):
        """ms per frame of one timed window from the seeded start state; variant: plain, judged, reactive."""
        d = ppamd.add_car_table(ppamd.alloc_scenes(S, 12, xp="torch", device=dev), xp="torch", device=dev)
        t = ppamd.alloc_traffic(S, xp="torch", device=dev)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev) if variant != "plain" else None
        follow = ppamd.alloc_follow(S, 12, xp="torch", device=dev) if variant == "reactive" else None
        b, T = ppamd.scene_struct(d), ppamd.traffic_struct(t)
        assert lib.pp_synth_traffic(h, 20261019, 0, C.byref(b), C.byref(T), 0, None) == 0
        R = ppamd.result_struct(res)
        J = ppamd.judge_struct(judge) if judge is not None else None
        F = ppamd.follow_struct(follow) if follow is not None else None

        def run(frames):
            cfg = ppamd.RolloutCfg(frames, a.consume, 300.0)
            args = (h, C.byref(b), C.byref(T), C.byref(prm), C.byref(cfg), C.byref(R), None, 0, None)
            if variant == "reactive":
                rc = lib.pp_rollout_reactive(*args, C.byref(jc), C.byref(J), C.byref(fc), C.byref(F))
            elif variant == "judged":
                rc = lib.pp_rollout_judged(*args, C.byref(jc), C.byref(J))
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
        if judge is not None:
            f = judge["flags"].cpu().numpy().view(np.uint32)
            rec = {k: int(((f >> i) & 1).sum()) for i, k in enumerate(ppamd.INC_KINDS)}
            rec["clean"] = int((f == 0).sum())
        if follow is not None:
            lead = follow["leader"].cpu().numpy()
            rec["cars_following_a_car"] = int(((lead >= 0) & (lead < 12)).sum())
            rec["cars_following_the_ego"] = int((lead == 12).sum())
        return ms, rec

    out = {"what": "ms per closed-loop frame, events on the launch stream; median of reps, variants alternating",
           "lib": os.path.basename(a.lib), "lib_sha256": ppamd.lib_sha256(a.lib), "gpu": torch.cuda.get_device_name(0),
           "frames": a.frames, "warmup": a.warmup, "consume": a.consume, "cars": 12, "reps": a.reps, "sizes": {}}
    variants = ["plain", "judged", "reactive"] if reactive_ok else ["plain"]
    for S in a.scenes:
        one(S, "plain")                                         # first touch of the size: workspace allocation
        ms = {v: [] for v in variants}
        rec = {}
        for _ in range(a.reps):
            for v in variants:
                m, rec[v] = one(S, v)
                ms[v].append(m)
        r = {"rollout_ms": statistics.median(ms["plain"]), "rollout_ms_all": ms["plain"]}
        if reactive_ok:
            cnt = follow_counts(12, ppamd.NUM_LANES)
            add = statistics.median(ms["reactive"]) - statistics.median(ms["judged"])
            r.update({"rollout_judged_ms": statistics.median(ms["judged"]), "rollout_judged_ms_all": ms["judged"],
                      "rollout_reactive_ms": statistics.median(ms["reactive"]), "rollout_reactive_ms_all": ms["reactive"],
                      "follow_ms": add, "follow_counts_per_scene": cnt,
                      "follow_GBps": (cnt["read"] + cnt["write"]) * S / (add * 1e-3) / 1e9 if add > 0 else None,
                      "follow_GFLOPs": cnt["flops"] * S / (add * 1e-3) / 1e9 if add > 0 else None,
                      "judged_scenes_with_incident": rec["judged"], "reactive_scenes_with_incident": rec["reactive"]})
        out["sizes"][str(S)] = r
        print(S, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "sizes"}))


if __name__ == "__main__":
    main()
