"""The sensor model's cost and a first study of what an imperfect sensor does to the drive (DESIGN.md
"Sensor model"). Writes profiles/sensor_drive.json.

(a) Cost: pp_rollout_lane_changing against pp_rollout_sensed per frame, with the identity sensor (no
Philox block is run: what the stage's reads and writes cost) and with a noisy one (noise, dropout and
occlusion all on), at 262,144 and 2,097,152 scenes of 12 cars, judge on, consume 3, from pp_synth_episode's
start. Every repetition starts each variant from the same episode start, runs 3 warm-up frames, then
times 20 frames between two events on the launch stream; the variants alternate and the median of 5
windows is reported as ms per frame, with the difference (what k_sense adds). Against it what the stage
needs per scene counted from csrc/pp_sensor.h (sensor_counts below): the bytes over the HBM peak, and
the Philox blocks the noisy sensor ran (from the last frame's fates) over the time it adds to the identity
sensor's, which also holds the occlusion pair tests. No time is fixed in advance.

(b) Study: pp_rollout_sweep_sensed over pos_sigma in {0, 0.25, 0.5, 1} x dropout_prob in {0, 0.1, 0.3}
(12 sets) at the default pp_params over the same seeded episodes; one summary row per set.

    python tools/sensor_drive.py
A run without a GPU fails; nothing here is an estimate."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "carnd-path-planning-project_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import ppamd  # noqa: E402
from sweep_drive import rows_of  # noqa: E402

SEED = 20261021
HBM_PEAK_GBS = 8000.0          # bench.py's figure: HBM3E 8.0 TB/s peak (spec)
NOISY = dict(seed=7, pos_sigma=0.5, pos_sigma_per_m=0.01, vel_sigma=0.5, dropout_prob=0.1, occlusion_radius=1.5)


def sensor_counts(n):
    """What k_sense needs per scene and frame with n truth rows, all reported (csrc/pp_sensor.h). Bytes:
    each address counted once (the occlusion loop's re-reads come from cache). philox_blocks: four
    Gaussians and the dropout word per row."""
    read = 2 * 8 + 4 + 4 + n * (4 + 4 * 8)                   # ego; n_cars, frame; the truth rows
    write = 4 + 4 + n * (4 + 4 * 8) + n * 4                  # n_cars, frame; the sensed rows; fate
    return {"read": read, "write": write, "cache_bytes": n * (n - 1) * 16, "philox_blocks": 5 * n,
            "pair_tests": n * (n - 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--study-scenes", type=int, default=262144, help="episodes driven per sensor setting")
    ap.add_argument("--study-frames", type=int, default=100)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sensor_drive.json"))
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "sensor_drive.py measures on a GPU"
    dev = torch.device("cuda", 0)
    wx, wy = ppamd.highway_map()
    m = ppamd.Map(wx, wy)
    n = 12
    out = {"what": "ms per closed-loop frame of pp_rollout_lane_changing and pp_rollout_sensed, events on the launch "
                   "stream, median of reps, variants alternating; a sweep over sensor settings",
           "lib_sha256": ppamd.lib_sha256(), "gpu": torch.cuda.get_device_name(0), "seed": SEED, "cars": n,
           "consume": a.consume, "frames": a.frames, "warmup": a.warmup, "reps": a.reps,
           "noisy_sensor": NOISY, "counts_per_scene": sensor_counts(n), "sizes": {}}

    # ---- (a) cost -------------------------------------------------------------------------------------
    prm = ppamd.default_params(n_speeds=1)
    sensors = {"changing": None, "identity": ppamd.default_sensor_cfg(), "noisy": ppamd.default_sensor_cfg(**NOISY)}

    def one(S, variant):
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        follow = ppamd.alloc_follow(S, n, xp="torch", device=dev)
        change = ppamd.alloc_lane_change(S, n, xp="torch", device=dev)
        sensor = ppamd.alloc_sensor(S, n, xp="torch", device=dev)
        d, t = ppamd.synth_episode(m, S, seed=SEED, device=0, judge=judge, follow=follow)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)

        def run(frames):
            if variant == "changing":
                ppamd.rollout_lane_changing(m, d, t, prm, res, follow, change, frames, a.consume, 300.0, judge=judge)
            else:
                ppamd.rollout_sensed(m, d, t, prm, res, follow, change, sensor, frames, a.consume, 300.0, judge=judge,
                                     scfg=sensors[variant])

        run(a.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(a.frames)
        e1.record()
        torch.cuda.synchronize()
        rec = None
        if variant != "changing":
            fate = sensor["fate"].cpu().numpy()
            rows = int((fate != 0).sum())
            rec = {"truth_rows_last_frame": rows, "reported": int((fate == 1).sum()), "occluded": int((fate == 2).sum()),
                   "dropped": int((fate == 3).sum())}
        return e0.elapsed_time(e1) / a.frames, rec

    cnt = sensor_counts(n)
    for S in a.scenes:
        one(S, "changing")                                       # first touch of the size: workspace allocation
        ms = {v: [] for v in sensors}
        rec = {}
        for _ in range(a.reps):
            for v in sensors:
                x, rec[v] = one(S, v)
                ms[v].append(x)
        med = {v: statistics.median(ms[v]) for v in sensors}
        r = {"rollout_lane_changing_ms": med["changing"], "rollout_lane_changing_ms_all": ms["changing"]}
        for v in ("identity", "noisy"):
            add = med[v] - med["changing"]
            r[v] = {"rollout_sensed_ms": med[v], "rollout_sensed_ms_all": ms[v], "sense_ms": add,
                    "share_of_frame": add / med["changing"], "fates_last_frame": rec[v],
                    "GB_per_s": (cnt["read"] + cnt["write"]) * S / add / 1e6 if add > 0 else None,
                    "of_hbm_peak": (cnt["read"] + cnt["write"]) * S / add / 1e6 / HBM_PEAK_GBS if add > 0 else None}
        draws = r["noisy"]["sense_ms"] - r["identity"]["sense_ms"]
        r["bytes_at_hbm_peak_ms"] = (cnt["read"] + cnt["write"]) * S / HBM_PEAK_GBS / 1e6
        r["noisy_minus_identity_ms"] = draws
        # blocks the noisy sensor ran in the last frame: the dropout block of every row that is not occluded,
        # four Gaussians per reported row; the pair tests: every ordered pair of a scene's rows
        f = rec["noisy"]
        blocks = f["reported"] + f["dropped"] + 4 * f["reported"]
        r["philox_blocks_last_frame"] = blocks
        r["philox_blocks_per_scene"] = blocks / S
        r["philox_blocks_per_s_if_all_of_the_difference"] = blocks / (draws * 1e-3) if draws > 0 else None
        r["sits_on"] = ("arithmetic (the Philox blocks and the occlusion pair tests)"
                        if draws > r["identity"]["sense_ms"] else "memory")
        out["sizes"][str(S)] = r
        print(S, json.dumps(r), flush=True)

    # ---- (b) the study ----------------------------------------------------------------------------------
    names, scfgs = [], []
    for sig in (0.0, 0.25, 0.5, 1.0):
        for p in (0.0, 0.1, 0.3):
            names.append({"pos_sigma": sig, "dropout_prob": p})
            scfgs.append(ppamd.default_sensor_cfg(seed=SEED, pos_sigma=sig, dropout_prob=p))
    S, F = a.study_scenes, a.study_frames
    hist_max = 25.0 * 0.02 * a.consume * F                   # what 25 m/s covers in the drive
    stats, _ = ppamd.rollout_sweep(m, [ppamd.default_params()] * len(scfgs), S, F, seed=SEED, consume=a.consume,
                                   hist_bins=a.bins, hist_max=hist_max, sensors=scfgs)
    torch.cuda.synchronize()
    rows = rows_of(stats, hist_max)
    out["study"] = {"scenes_per_set": S, "frames": F, "hist_bins": a.bins, "hist_max_m": hist_max,
                    "params": "pp_params_default", "sets": [dict(nm, row=rows[p]) for p, nm in enumerate(names)]}
    for nm, r in zip(names, rows):
        print(json.dumps(dict(nm, clean_share=r["n_clean"] / r["n_scenes"], clean_dist_mean_m=r["clean_dist_mean_m"],
                              dist_mean_m=r["dist_mean_m"], collided=r["scenes_with"][0], speed=r["scenes_with"][1],
                              acc=r["scenes_with"][2], jerk=r["scenes_with"][3], off_lane=r["scenes_with"][4],
                              min_sep=r["min_sep"], max_jerk=r["max_jerk"])), flush=True)

    def plain(o):                                        # strict JSON: "inf" / "-inf" / "nan" as strings
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        return str(o) if isinstance(o, float) and not np.isfinite(o) else o

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(plain(out), open(a.out, "w"), indent=1, allow_nan=False)


if __name__ == "__main__":
    main()
