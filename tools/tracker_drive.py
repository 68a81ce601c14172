"""The tracker's cost and a first study of what tracking does to a drive behind an imperfect sensor
(DESIGN.md "Tracker"). Writes profiles/tracker_drive.json.

(a) Cost: pp_rollout_sensed against pp_rollout_tracked per frame behind the same noisy sensor, with the
identity tracker (every row taken outright: what the stage's reads and writes cost) and with a matched
filter that coasts, at 262,144 and 2,097,152 scenes of 12 cars, judge on, consume 3, from
pp_synth_episode's start. Every repetition starts each variant from the same episode start, runs 3
warm-up frames, then times 20 frames between two events on the launch stream; the variants alternate and
the median of 5 windows is reported as ms per frame, with the difference (what k_track adds). Against it
what the stage needs per scene counted from csrc/pp_tracker.h (tracker_counts below) over the HBM peak.
No time is fixed in advance.

(b) Study: pp_rollout_sweep_tracked over pos_sigma in {0.5, 1} x dropout_prob in {0, 0.3}, each with the
identity tracker and with a matched filter that coasts (8 sets) at the default pp_params over the same
seeded episodes; one summary row per set. Whether tracking helps the judged drive is the finding.

(c) Probes of that finding at pos_sigma 0.5 without dropout: the same two trackers with lane changes off,
and two filters that trust the reported velocity or the constant-velocity model less.

    python tools/tracker_drive.py
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
MATCHED = dict(meas_pos_sigma=0.5, meas_pos_sigma_per_m=0.01, meas_vel_sigma=0.5, acc_sigma=1.0, max_coast=5)
STUDY_ACC_SIGMA, STUDY_MAX_COAST = 1.0, 10


def tracker_counts(n):
    """What k_track needs per scene and frame with n slots, n rows reported and n old tracks, all updated
    (csrc/pp_tracker.h). Each address counted once."""
    slot, row = 4 + 4 + 7 * 8, 4 + 4 * 8                     # id, misses, state, covariance; id and four values
    read = 2 * 8 + 4 + 4 + 4 + n * row + n * slot            # ego; n_cars, frame, n_tracks; the rows; the old bank
    write = 4 + 4 + 4 + n * slot + n * row + n * 4           # frame, n_tracks, n_cars; the new bank; the rows; src
    return {"read": read, "write": write}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--study-scenes", type=int, default=262144, help="episodes driven per setting")
    ap.add_argument("--study-frames", type=int, default=100)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tracker_drive.json"))
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "tracker_drive.py measures on a GPU"
    dev = torch.device("cuda", 0)
    wx, wy = ppamd.highway_map()
    m = ppamd.Map(wx, wy)
    n = 12
    out = {"what": "ms per closed-loop frame of pp_rollout_sensed and pp_rollout_tracked, events on the launch "
                   "stream, median of reps, variants alternating; a sweep over sensor and tracker settings",
           "lib_sha256": ppamd.lib_sha256(), "gpu": torch.cuda.get_device_name(0), "seed": SEED, "cars": n,
           "consume": a.consume, "frames": a.frames, "warmup": a.warmup, "reps": a.reps,
           "sensor": NOISY, "matched_tracker": MATCHED, "counts_per_scene": tracker_counts(n), "sizes": {}}

    # ---- (a) cost -------------------------------------------------------------------------------------
    prm = ppamd.default_params(n_speeds=1)
    scfg = ppamd.default_sensor_cfg(**NOISY)
    trackers = {"sensed": None, "identity": ppamd.default_tracker_cfg(), "matched": ppamd.default_tracker_cfg(**MATCHED)}

    def one(S, variant):
        judge = ppamd.alloc_judge(S, xp="torch", device=dev)
        follow = ppamd.alloc_follow(S, n, xp="torch", device=dev)
        change = ppamd.alloc_lane_change(S, n, xp="torch", device=dev)
        sensor = ppamd.alloc_sensor(S, n, xp="torch", device=dev)
        tracker = ppamd.alloc_tracker(S, n, xp="torch", device=dev)
        d, t = ppamd.synth_episode(m, S, seed=SEED, device=0, judge=judge, follow=follow)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)

        def run(frames):
            if variant == "sensed":
                ppamd.rollout_sensed(m, d, t, prm, res, follow, change, sensor, frames, a.consume, 300.0, judge=judge,
                                     scfg=scfg)
            else:
                ppamd.rollout_tracked(m, d, t, prm, res, follow, change, sensor, tracker, frames, a.consume, 300.0,
                                      judge=judge, scfg=scfg, tcfg=trackers[variant])

        run(a.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(a.frames)
        e1.record()
        torch.cuda.synchronize()
        rec = None
        if variant != "sensed":
            src = tracker["src"].cpu().numpy()
            rec = {"new": int((src == 1).sum()), "updated": int((src == 2).sum()), "coasted": int((src == 3).sum())}
        return e0.elapsed_time(e1) / a.frames, rec

    cnt = tracker_counts(n)
    for S in a.scenes:
        one(S, "sensed")                                         # first touch of the size: workspace allocation
        ms = {v: [] for v in trackers}
        rec = {}
        for _ in range(a.reps):
            for v in trackers:
                x, rec[v] = one(S, v)
                ms[v].append(x)
        med = {v: statistics.median(ms[v]) for v in trackers}
        r = {"rollout_sensed_ms": med["sensed"], "rollout_sensed_ms_all": ms["sensed"],
             "bytes_at_hbm_peak_ms": (cnt["read"] + cnt["write"]) * S / HBM_PEAK_GBS / 1e6}
        for v in ("identity", "matched"):
            add = med[v] - med["sensed"]
            r[v] = {"rollout_tracked_ms": med[v], "rollout_tracked_ms_all": ms[v], "track_ms": add,
                    "share_of_frame": add / med["sensed"], "src_last_frame": rec[v],
                    "GB_per_s": (cnt["read"] + cnt["write"]) * S / add / 1e6 if add > 0 else None,
                    "of_hbm_peak": (cnt["read"] + cnt["write"]) * S / add / 1e6 / HBM_PEAK_GBS if add > 0 else None}
        out["sizes"][str(S)] = r
        print(S, json.dumps(r), flush=True)

    # ---- (b) the study ----------------------------------------------------------------------------------
    names, scfgs, tcfgs = [], [], []
    for sig in (0.5, 1.0):
        for p in (0.0, 0.3):
            for tracked in (False, True):
                names.append({"pos_sigma": sig, "dropout_prob": p, "tracker": "matched" if tracked else "identity"})
                scfgs.append(ppamd.default_sensor_cfg(seed=SEED, pos_sigma=sig, dropout_prob=p))
                tcfgs.append(ppamd.default_tracker_cfg(meas_pos_sigma=sig, acc_sigma=STUDY_ACC_SIGMA,
                                                       max_coast=STUDY_MAX_COAST) if tracked
                             else ppamd.default_tracker_cfg())
    S, F = a.study_scenes, a.study_frames
    hist_max = 25.0 * 0.02 * a.consume * F                   # what 25 m/s covers in the drive
    stats, _ = ppamd.rollout_sweep(m, [ppamd.default_params()] * len(scfgs), S, F, seed=SEED, consume=a.consume,
                                   hist_bins=a.bins, hist_max=hist_max, sensors=scfgs, trackers=tcfgs)
    torch.cuda.synchronize()
    rows = rows_of(stats, hist_max)
    out["study"] = {"scenes_per_set": S, "frames": F, "hist_bins": a.bins, "hist_max_m": hist_max,
                    "params": "pp_params_default",
                    "matched_tracker": {"meas_pos_sigma": "the sensor's pos_sigma", "meas_vel_sigma": 0.0,
                                        "acc_sigma": STUDY_ACC_SIGMA, "max_coast": STUDY_MAX_COAST},
                    "sets": [dict(nm, row=rows[p]) for p, nm in enumerate(names)]}
    for nm, r in zip(names, rows):
        print(json.dumps(dict(nm, clean_share=r["n_clean"] / r["n_scenes"], clean_dist_mean_m=r["clean_dist_mean_m"],
                              dist_mean_m=r["dist_mean_m"], collided=r["scenes_with"][0], speed=r["scenes_with"][1],
                              acc=r["scenes_with"][2], jerk=r["scenes_with"][3], off_lane=r["scenes_with"][4],
                              min_sep=r["min_sep"], max_jerk=r["max_jerk"])), flush=True)

    # ---- (c) probes: where the matched filter's collisions come from ----------------------------------------
    # The simulator reports a car's velocity along its lane (ppsynth::traffic_car): a lane change moves the car
    # sideways at lateral_speed with no lateral velocity reported. At pos_sigma 0.5 without dropout: the study's
    # two trackers with lane changes off; and with lane changes on, the filter told to distrust the velocity
    # (meas_vel_sigma 1.5, the lane change's lateral speed) or the model (acc_sigma 10).
    def short(r):
        return {"clean_share": r["n_clean"] / r["n_scenes"], "collided": r["scenes_with"][0], "jerk": r["scenes_with"][3],
                "off_lane": r["scenes_with"][4], "clean_dist_mean_m": r["clean_dist_mean_m"]}

    one_s = ppamd.default_sensor_cfg(seed=SEED, pos_sigma=0.5)
    study_t = ppamd.default_tracker_cfg(meas_pos_sigma=0.5, acc_sigma=STUDY_ACC_SIGMA, max_coast=STUDY_MAX_COAST)
    probes = []
    for lane_changes, group in ((False, [("identity", ppamd.default_tracker_cfg()), ("matched", study_t)]),
                                (True, [("matched, meas_vel_sigma 1.5",
                                         ppamd.default_tracker_cfg(meas_pos_sigma=0.5, meas_vel_sigma=1.5,
                                                                   acc_sigma=STUDY_ACC_SIGMA, max_coast=STUDY_MAX_COAST)),
                                        ("matched, acc_sigma 10",
                                         ppamd.default_tracker_cfg(meas_pos_sigma=0.5, acc_sigma=10.0,
                                                                   max_coast=STUDY_MAX_COAST))])):
        stats, _ = ppamd.rollout_sweep(m, [ppamd.default_params()] * len(group), S, F, seed=SEED, consume=a.consume,
                                       hist_bins=a.bins, hist_max=hist_max, sensors=[one_s] * len(group),
                                       trackers=[t for _, t in group], lane_changes=lane_changes)
        torch.cuda.synchronize()
        for (name, _), r in zip(group, rows_of(stats, hist_max)):
            probes.append(dict({"pos_sigma": 0.5, "dropout_prob": 0.0, "lane_changes": lane_changes, "tracker": name},
                               **short(r)))
            print(json.dumps(probes[-1]), flush=True)
    out["probes"] = probes

    def plain(o):                                       # strict JSON: "inf" / "-inf" / "nan" as strings
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        return str(o) if isinstance(o, float) and not np.isfinite(o) else o

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(plain(out), open(a.out, "w"), indent=1, allow_nan=False)


if __name__ == "__main__":
    main()
