"""What a judged, reactive drive records from each start state (DESIGN.md "Episode starts"):
pp_rollout_reactive with the judge for 100 frames on one GPU at 262,144 and 2,097,152 scenes, 12 cars,
consume 3, once from pp_synth_traffic (the benchmark's snapshot) and once from pp_synth_episode,
alternating, two runs of each.

Every frame is one pp_rollout_reactive call between two events on the launch stream, so the time per
frame is known frame by frame: reported as the median of frames 4-13 and of frames 50-99 separately
(DESIGN.md §15 found the planner's checked candidate kernel at 3 ms from frame 14 on with the old
start). Also: the incident census per kind (scenes, earliest driven step, all from the judge state),
the median clean_dist, the slowest traffic speed reached in the drive, and the generator's own time
(events around its launch, median of 5 after one untimed call). Writes profiles/episode_drive.json,
stamped with the SHA-256 of the library measured.

    python tools/episode_drive.py
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
import ppamd  # noqa: E402

SEED = 20261020


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "episode_drive.json"))
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "episode_drive.py measures on a GPU"
    dev = torch.device("cuda", 0)
    wx, wy = ppamd.highway_map()
    m = ppamd.Map(wx, wy)
    prm = ppamd.default_params(n_speeds=1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def start(S, kind):
        """(scenes, traffic, judge, follow, generator ms, step offset)"""
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        follow = ppamd.alloc_follow(S, 12, xp="torch", device=dev)
        d = ppamd.add_car_table(ppamd.alloc_scenes(S, 12, xp="torch", device=dev), xp="torch", device=dev)
        t = ppamd.alloc_traffic(S, xp="torch", device=dev)
        b, T = ppamd.scene_struct(d), ppamd.traffic_struct(t)
        if kind == "episode":
            cfg, J, F = ppamd.default_episode_cfg(), ppamd.judge_struct(judge), ppamd.follow_struct(follow)
            ms, rc = timed(lambda: ppamd.lib.pp_synth_episode(m.handle, SEED, 0, C.byref(cfg), None, C.byref(b),
                                                              C.byref(T), C.byref(J), C.byref(F), 0, None))
        else:
            ms, rc = timed(lambda: ppamd.lib.pp_synth_traffic(m.handle, SEED, 0, C.byref(b), C.byref(T), 0, None))
        assert rc == 0, rc
        t["n_cars"] = T.n_cars
        return d, t, judge, follow, ms, ppamd.JUDGE_RING if kind == "episode" else 0

    def generator_ms(S, kind):
        start(S, kind)
        return statistics.median(start(S, kind)[4] for _ in range(5))

    def drive(S, kind):
        ppamd.plan_reset(m)
        d, t, judge, follow, _, off = start(S, kind)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        ms, slowest = [], float("inf")
        stood = torch.zeros(S, dtype=torch.bool, device=dev)          # scenes in which a car came to rest
        for _ in range(a.frames):
            dt, _ = timed(lambda: ppamd.rollout_reactive(m, d, t, prm, res, follow, 1, a.consume, 300.0, judge=judge))
            ms.append(dt)
            slowest = min(slowest, float(t["speed"][:t["n_cars"]].min()))
            stood |= (t["speed"][:t["n_cars"]] == 0).any(dim=0)
        j = ppamd.judge_to_numpy(judge)
        assert (j["steps"] == off + a.frames * a.consume).all()
        kinds = {}
        for i, k in enumerate(ppamd.INC_KINDS):
            fs = j["first_step"][i]
            kinds[k] = {"scenes": int((fs > 0).sum()),
                        "earliest_driven_step": int(fs[fs > 0].min()) - off if (fs > 0).any() else None}
        first_any = np.where(j["first_step"] > 0, j["first_step"], np.iinfo(np.int32).max).min(axis=0)
        return {"start": kind, "scenes_with_any_incident": int((j["flags"] != 0).sum()),
                "earliest_driven_step_any": int(first_any.min()) - off if (j["flags"] != 0).any() else None,
                "kinds": kinds, "clean_dist_median_m": float(np.nanmedian(j["clean_dist"])),
                "dist_median_m": float(np.nanmedian(j["dist"])),
                "scenes_with_a_non_finite_dist": int((~np.isfinite(j["dist"])).sum()),
                "slowest_traffic_speed_mps": slowest, "scenes_in_which_a_car_came_to_rest": int(stood.sum()),
                "cars_at_rest_at_the_end": int((t["speed"][:t["n_cars"]] == 0).sum()),
                "frame_ms_median_4_13": statistics.median(ms[4:14]),
                "frame_ms_median_50_99": statistics.median(ms[50:100]) if a.frames >= 100 else None,
                "frame_ms": [round(x, 4) for x in ms]}

    out = {"what": "pp_rollout_reactive with the judge, one call per frame between events on the launch stream; "
                   "starts alternating",
           "lib_sha256": ppamd.lib_sha256(), "gpu": torch.cuda.get_device_name(0), "frames": a.frames,
           "consume": a.consume, "cars": 12, "seed": SEED, "sizes": {}}
    for S in a.scenes:
        drive(S, "traffic")                                     # first touch of the size: workspace allocation
        runs = []
        for _ in range(a.runs):
            for kind in ("traffic", "episode"):
                runs.append(drive(S, kind))
                print(S, json.dumps({k: v for k, v in runs[-1].items() if k != "frame_ms"}), flush=True)
        gen = {kind: generator_ms(S, kind) for kind in ("traffic", "episode")}
        print(S, "generator ms", json.dumps(gen), flush=True)
        out["sizes"][str(S)] = {"generator_ms": gen, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
