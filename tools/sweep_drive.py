"""A parameter sweep of the planner, judged and summarised on the GPU (DESIGN.md "Judge summary and
parameter sweeps"): pp_rollout_sweep drives the same seeded episodes of lane-changing traffic once per
parameter set, keep_distance in {5, 10, 20, 30} x cost_mode in {reference, comfort} (8 sets), and
leaves one row of figures per set and group on the device. The rows are copied to the host once, at
the end, and written to profiles/sweep_drive.json with the sweep's wall time.

The summary's own time is measured at 262,144 and 2,097,152 scenes on the judge state a short drive
leaves: events on the stream around pp_judge_summary, one untimed call, median of 5, for one group of
all scenes, 8 groups and groups of 100 scenes (rows written by the tile kernel). Against it the bytes
counted from the code (96 B read per scene: steps, flags, 5 counts, 5 first steps, 6 doubles; the rows
and tile records written) over that time and the HBM peak, and, in the same run, what the summary
replaces: the same arrays copied to the host and reduced with NumPy to the same figures (wall clock,
one untimed pass, median of 5). No time is fixed in advance.

    python tools/sweep_drive.py
A run without a GPU fails; nothing here is an estimate."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "carnd-path-planning-project_amd"))

import numpy as np  # noqa: E402
import ppamd  # noqa: E402

SEED = 20261021
HBM_PEAK_GBS = 8000.0          # bench.py's figure: HBM3E 8.0 TB/s peak (spec)
SCENE_BYTES = 4 + 4 + 4 * 5 + 4 * 5 + 8 * 6      # what k_summary_tiles reads of a scene
ROW_BYTES = 8 * 5 + 8 * 5 * 2 + 4 * 5 + 8 * 8    # a row without its histogram
REC_BYTES = 200                                  # a chunk's part (ppsummary::Part); 16 B more per tile (T_t)
READ = ["steps", "flags", "count", "first_step", "dist", "clean_dist", "min_sep", "max_speed_mph", "max_acc",
        "max_jerk"]


def numpy_rows(j, S, E, B, hist_max):
    """The summary's figures from host arrays, group by group, the plain NumPy way."""
    rows = []
    inv_w = B / hist_max
    for a in range(0, S, E):
        sl = slice(a, min(S, a + E))
        steps, dist, clean = j["steps"][sl], j["dist"][sl], j["clean_dist"][sl]
        judged = steps != 0
        fin = judged & np.isfinite(dist) & np.isfinite(clean)
        cnt, fs = j["count"][:, sl], j["first_step"][:, sl]
        q = clean[fin] * inv_w
        rows.append({
            "n_scenes": len(steps), "n_unjudged": int((~judged).sum()), "n_nonfinite": int((judged & ~fin).sum()),
            "n_clean": int((judged & (j["flags"][sl] == 0)).sum()), "steps": int(steps[judged].sum(dtype=np.int64)),
            "scenes_with": ((cnt > 0) & judged).sum(1).tolist(),
            "steps_in": np.where(judged, cnt, 0).sum(1, dtype=np.int64).tolist(),
            "first_step_min": np.where(judged & (fs > 0), fs, np.iinfo(np.int32).max).min(1).tolist(),
            "dist_sum": float(dist[fin].sum()), "clean_dist_sum": float(clean[fin].sum()),
            "clean_dist_min": float(clean[fin].min()) if fin.any() else float("inf"),
            "clean_dist_max": float(clean[fin].max()) if fin.any() else float("-inf"),
            "min_sep": float(np.fmin.reduce(j["min_sep"][sl][judged], initial=np.inf)),
            "max_speed_mph": float(np.fmax.reduce(j["max_speed_mph"][sl][judged], initial=-np.inf)),
            "max_acc": float(np.fmax.reduce(j["max_acc"][sl][judged], initial=-np.inf)),
            "max_jerk": float(np.fmax.reduce(j["max_jerk"][sl][judged], initial=-np.inf)),
            "hist": np.bincount(np.where(q >= B - 1, B - 1, q.astype(np.int64)), minlength=B).tolist()})
    return rows


def rows_of(stats, hist_max):
    """The stats arrays as a list of rows (plain Python numbers), with the median's and the 10 % and 90 %
    quantiles' bins."""
    st = ppamd.stats_to_numpy(stats)
    out = []
    for r in range(st["n_scenes"].shape[0]):
        row = {k: (v[..., r].tolist() if v.ndim > 1 else (float(v[r]) if v.dtype.kind == "f" else int(v[r])))
               for k, v in st.items()}
        n = row["n_scenes"] - row["n_unjudged"] - row["n_nonfinite"]
        row["dist_mean_m"] = row["dist_sum"] / n if n else None
        row["clean_dist_mean_m"] = row["clean_dist_sum"] / n if n else None
        for q in (0.1, 0.5, 0.9):
            row[f"clean_dist_q{int(q * 100)}_bin_m"] = list(ppamd.stats_quantile(st, r, q, hist_max))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep-scenes", type=int, default=262144, help="episodes driven per parameter set")
    ap.add_argument("--groups", type=int, default=4, help="groups (rows) per set")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--consume", type=int, default=3)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--cost-scenes", type=int, nargs="+", default=[262144, 2097152])
    ap.add_argument("--cost-frames", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweep_drive.json"))
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "sweep_drive.py measures on a GPU"
    dev = torch.device("cuda", 0)
    wx, wy = ppamd.highway_map()
    m = ppamd.Map(wx, wy)

    out = {"what": "pp_rollout_sweep over lane-changing traffic from pp_synth_episode; pp_judge_summary's own time "
                   "against the host copy and NumPy reduction it replaces",
           "lib_sha256": ppamd.lib_sha256(), "gpu": torch.cuda.get_device_name(0), "seed": SEED, "cars": 12,
           "consume": a.consume}

    # ---- the sweep ----------------------------------------------------------------------------------
    names, sets = [], []
    for mode, mname in ((ppamd.COST_REFERENCE, "reference"), (ppamd.COST_COMFORT, "comfort")):
        for kd in (5.0, 10.0, 20.0, 30.0):
            p = ppamd.default_params(cost_mode=mode)
            p.keep_distance = kd
            sets.append(p)
            names.append({"keep_distance": kd, "cost_mode": mname})
    S, G = a.sweep_scenes, a.groups
    E = -(-S // G)
    hist_max = 25.0 * 0.02 * a.consume * a.frames          # what 25 m/s covers in the drive
    sweep_ms = []
    stats = buf = None
    for _ in range(2):                                     # the first touch of the size allocates
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats, buf = ppamd.rollout_sweep(m, sets, S, a.frames, scenes_per_group=E, seed=SEED, consume=a.consume,
                                         hist_bins=a.bins, hist_max=hist_max, buffers=buf)
        torch.cuda.synchronize()
        sweep_ms.append((time.perf_counter() - t0) * 1e3)
    rows = rows_of(stats, hist_max)
    out["sweep"] = {"scenes_per_set": S, "groups_per_set": G, "scenes_per_group": E, "frames": a.frames,
                    "hist_bins": a.bins, "hist_max_m": hist_max, "wall_ms_first_and_second_call": sweep_ms,
                    "sets": [dict(n, rows=rows[p * G:(p + 1) * G]) for p, n in enumerate(names)]}
    for p, n in enumerate(names):
        rs = rows[p * G:(p + 1) * G]
        tot = sum(r["n_scenes"] for r in rs)
        print(json.dumps(dict(n, clean_share=sum(r["n_clean"] for r in rs) / tot,
                              clean_dist_mean_m=sum(r["clean_dist_sum"] for r in rs) / tot,
                              collided=sum(r["scenes_with"][0] for r in rs),
                              jerk=sum(r["scenes_with"][3] for r in rs))), flush=True)
    print("sweep wall ms", sweep_ms, flush=True)
    del buf, stats

    # ---- the summary's own cost -----------------------------------------------------------------------
    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out["summary_cost"] = {}
    B, hm = a.bins, 25.0 * 0.02 * a.consume * a.cost_frames
    for S in a.cost_scenes:
        prm = ppamd.default_params(n_speeds=1)
        judge, follow = ppamd.alloc_judge(S, xp="torch", device=dev), ppamd.alloc_follow(S, 12, xp="torch", device=dev)
        lc = ppamd.alloc_lane_change(S, 12, xp="torch", device=dev)
        d, g = ppamd.synth_episode(m, S, seed=SEED, device=0, judge=judge, follow=follow)
        res = ppamd.alloc_result(S, prm, xp="torch", device=dev)
        ppamd.rollout_lane_changing(m, d, g, prm, res, follow, lc, a.cost_frames, a.consume, 300.0, judge=judge)
        torch.cuda.synchronize()
        del d, g, res, follow, lc
        size = {}
        for label, E in (("one_group", S), ("8_groups", -(-S // 8)), ("groups_of_100", 100)):
            G = -(-S // E)
            tpg = -(-min(E, S) // 256)
            tiles = G * tpg
            K = min(max(1, min(8, tiles // 512)), tpg)       # the library's tiles per chunk (summary_args)
            chunks = G * -(-tpg // K)
            st = ppamd.alloc_judge_stats(G, B, xp="torch", device=dev)
            call = lambda: ppamd.judge_summary(judge, S, E, hist_bins=B, hist_max=hm, m=m, stats=st)  # noqa: E731
            events(call)
            ms = sorted(events(call) for _ in range(5))
            recs = 2 * (chunks * REC_BYTES + tiles * 16) if tpg > 1 else 0      # written, then read
            nbytes = S * SCENE_BYTES + G * (ROW_BYTES + 8 * B) * 2 + recs
            size[label] = {"groups": G, "tiles": tiles, "tiles_per_chunk": K, "ms_median_of_5": ms[2], "ms_all": ms,
                           "counted_bytes": nbytes, "GB_per_s": nbytes / ms[2] / 1e6,
                           "of_hbm_peak": nbytes / ms[2] / 1e6 / HBM_PEAK_GBS}
            print(S, label, json.dumps(size[label]), flush=True)
            dev_rows = ppamd.stats_to_numpy(st)

            def host_way():
                t0 = time.perf_counter()
                jh = {k: judge[k].cpu().numpy() for k in READ}
                t1 = time.perf_counter()
                r = numpy_rows(jh, S, E, B, hm)
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, r

            if label != "groups_of_100" or S <= 262144:      # (a Python loop over 20,972 groups measures Python)
                host_way()
                runs = [host_way() for _ in range(5)]
                cp, red = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
                hr = runs[-1][2]
                same = all(hr[g]["n_clean"] == int(dev_rows["n_clean"][g]) and
                           hr[g]["hist"] == dev_rows["hist"][:, g].tolist() and
                           abs(hr[g]["clean_dist_sum"] - dev_rows["clean_dist_sum"][g]) <=
                           1e-9 * abs(hr[g]["clean_dist_sum"]) for g in range(G))
                size[label]["host_copy_ms"] = cp
                size[label]["numpy_reduce_ms"] = red
                size[label]["host_bytes_copied"] = S * SCENE_BYTES
                size[label]["host_agrees"] = bool(same)
                print(S, label, "host copy ms", round(cp, 3), "numpy ms", round(red, 3), "agrees", same, flush=True)
        out["summary_cost"][str(S)] = size
        del judge
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
