"""What the rollout judge costs per frame (DESIGN.md "Rollout judge"): pp_rollout against
pp_rollout_judged on one GPU at 262,144 and 2,097,152 scenes, 12 cars, consume 3.

Every repetition starts both variants from the same synthetic start state (pp_synth_traffic, one
seed), runs 3 warm-up frames, then times 20 frames between two events on the launch stream; the
variants alternate and the median of the repetitions is reported as ms per frame, with the
difference (what k_judge adds), the bytes k_judge moves per scene counted from csrc/pp_judge.h
(judge_bytes below) and the rate that makes. Writes profiles/judge_cost.json, stamped with the
SHA-256 of the library measured.

    python tools/judge_cost.py                      # this build, both sizes
    python tools/judge_cost.py --lib OTHER.so --plain-only --out parent.json
                                                    # pp_rollout alone of another build (a parent
                                                    # commit's library has no judge)
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


def judge_bytes(n_cars, consume, cfg):
    """Bytes k_judge reads and writes per scene and frame in steady state (csrc/pp_judge.h), each
    address counted once per frame (the consume re-reads of the traffic come from cache)."""
    ego = 3 * 8 + 4                                            # ego_x, ego_y, ego_yaw_deg, n_out
    plan = consume * 2 * 8
    traffic = n_cars * (4 + 4 + 8 + 8 + 8)                      # lane, seg, t, offset, speed
    ring_w = consume * 2 * 8
    ring_r = 3 * consume * 2 * 8                                # v_{n-Wa}, v_{n-Wj}, v_{n-Wj-Wa}
    state = 4 + 4 + 2 * len(ppamd.INC_KINDS) * 4 + 3 * 4 + 8 * 8   # steps, flags, records, carried ints, 8 doubles
    return {"read": ego + plan + traffic + ring_r + state, "write": ring_w + state}


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
    if hasattr(lib, "pp_rollout_judged"):
        lib.pp_rollout_judged.argtypes = lib.pp_rollout.argtypes + [C.POINTER(ppamd.JudgeCfg), C.POINTER(ppamd.Judge)]
        lib.pp_judge_cfg_default.argtypes = [C.POINTER(ppamd.JudgeCfg)]
        lib.pp_judge_cfg_default.restype = None
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
    ap.add_argument("--out", help="default profiles/judge_cost.json; required with --lib or --plain-only")
    a = ap.parse_args()
    if a.out is None:
        if a.plain_only or os.path.abspath(a.lib) != os.path.abspath(ppamd.LIB_PATH):
            ap.error("--out is required with --lib or --plain-only (profiles/judge_cost.json is this build's record)")
        a.out = os.path.join(REPO, "profiles", "judge_cost.json")

    import torch
    assert torch.cuda.is_available(), "judge_cost.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lib = open_lib(a.lib)
    judged_ok = hasattr(lib, "pp_rollout_judged") and not a.plain_only
    wx, wy = ppamd.highway_map()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert lib.pp_map_create(wx.ctypes.data_as(dp), wy.ctypes.data_as(dp), len(wx), C.byref(h)) == 0
    prm = ppamd.Params()
    lib.pp_params_default(C.byref(prm))
    prm.n_speeds, prm.n_points = 1, 50
    jc = ppamd.JudgeCfg()
    if judged_ok:
        lib.pp_judge_cfg_default(C.byref(jc))

    def one(S, judged):
        """ms per frame of one timed window from the seeded start state."""
        d = ppamd.add_car_table(ppamd.alloc_scenes(S, 12, xp="torch", device=dev), xp="torch", device=dev)
        t = ppamd.alloc_traffic(S, xp="torch", device=dev)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        judge = ppamd.alloc_judge(S, xp="torch", device=dev) if judged else None
        b, T = ppamd.scene_struct(d), ppamd.traffic_struct(t)
        assert lib.pp_synth_traffic(h, 20261019, 0, C.byref(b), C.byref(T), 0, None) == 0
        R = ppamd.result_struct(res)
        J = ppamd.judge_struct(judge) if judged else None

        def run(frames):
            cfg = ppamd.RolloutCfg(frames, a.consume, 300.0)
            if judged:
                rc = lib.pp_rollout_judged(h, C.byref(b), C.byref(T), C.byref(prm), C.byref(cfg), C.byref(R), None, 0,
                                           None, C.byref(jc), C.byref(J))
            else:
                rc = lib.pp_rollout(h, C.byref(b), C.byref(T), C.byref(prm), C.byref(cfg), C.byref(R), None, 0, None)
            assert rc == 0, rc

        run(a.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(a.frames)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.frames
        flags = None
        if judged:
            f = judge["flags"].cpu().numpy().view(np.uint32)
            flags = {k: int(((f >> i) & 1).sum()) for i, k in enumerate(ppamd.INC_KINDS)}
            flags["clean"] = int((f == 0).sum())
        return ms, flags

    out = {"what": "ms per closed-loop frame, events on the launch stream; median of reps, variants alternating",
           "lib": os.path.basename(a.lib), "lib_sha256": ppamd.lib_sha256(a.lib), "gpu": torch.cuda.get_device_name(0),
           "frames": a.frames, "warmup": a.warmup, "consume": a.consume, "cars": 12, "reps": a.reps, "sizes": {}}
    for S in a.scenes:
        one(S, False)                                           # first touch of the size: workspace allocation
        plain, judged, flags = [], [], None
        for _ in range(a.reps):
            plain.append(one(S, False)[0])
            if judged_ok:
                ms, flags = one(S, True)
                judged.append(ms)
        r = {"rollout_ms": statistics.median(plain), "rollout_ms_all": plain}
        if judged_ok:
            by = judge_bytes(12, a.consume, jc)
            add = statistics.median(judged) - r["rollout_ms"]
            r.update({"rollout_judged_ms": statistics.median(judged), "rollout_judged_ms_all": judged,
                      "judge_ms": add, "judge_bytes_per_scene": by,
                      "judge_GBps": (by["read"] + by["write"]) * S / (add * 1e-3) / 1e9 if add > 0 else None,
                      "scenes_with_incident": flags})
        out["sizes"][str(S)] = r
        print(S, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "sizes"}))


if __name__ == "__main__":
    main()
