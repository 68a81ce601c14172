"""bench.py's plain run and --dump-outputs: a plain run carries the headline fields and none of the
side measurements that --full adds; --dump-outputs writes what the last timed step left in the
caller's result buffers, as float64 .npy files, whole or as a fixed seeded sample of the scenes,
identical from run to run. The sample arithmetic is checked on the CPU; on the GPU the dumped rows
must equal a direct pp_eval of the same seeded scenes bit for bit."""
import json

import numpy as np
import pytest

import bench
import oracle_lib
from oracle_lib import ppamd

SIDE_KEYS = ("pcie_inclusive", "weak_scaling", "shard_projection", "comfort", "cpu_baseline")


def test_options_default_off():
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "d"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, True, "d")


@pytest.mark.parametrize("S,per_scene,budget", [(10, 952, 1 << 20), (3001, 952, 952 * 1000), (2_097_152, 952, 48 << 20),
                                                (262_144, 38_800, 48 << 20), (5, 100, 250)])
def test_dump_sample_fits_budget_and_repeats(S, per_scene, budget):
    idx = bench.dump_sample(S, per_scene, budget)
    assert idx.dtype == np.int64 and 1 <= len(idx) <= S
    assert len(idx) == S or len(idx) * per_scene <= budget
    assert len(idx) == min(S, max(1, budget // per_scene))
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < S      # sorted, distinct, in range
    assert np.array_equal(idx, bench.dump_sample(S, per_scene, budget))   # the same sample every run


def test_default_dump_stays_under_64_mb():
    # BASELINE configs 5, 3 and 4 as alloc_result shapes them: float64 elements per scene
    for S, per in ((2_097_152, 2 + 2 * 50 + 15 + 1), (262_144, 2 + 2 * 100 + 24 + 1 + 100 * 24 * 2 + 24),
                   (16_384, 2 + 2 * 50 + 192 + 1 + 3)):
        k = len(bench.dump_sample(S, per * 8 + 8, bench.DUMP_BUDGET_BYTES))
        # every file's .npy header is 128 bytes
        assert k * (per * 8 + 8) + 16 * 128 <= 64 * 1000 * 1000


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [False, True])
def test_plain_run_dumps_last_step(tmp_path, capsys, monkeypatch, sampled):
    import torch
    S = 3001
    if sampled:
        monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 952 * 1000)
    assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--scenes", str(S),
                       "--dump-outputs", str(tmp_path)]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["value"] == pytest.approx(S * 15 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["unit"] == "candidate trajectories/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert not any(k in out for k in SIDE_KEYS)
    assert out["kernels_ms_avg"]["k_cand"] > 0 and out["kernels_ms_avg"]["k_prep"] is None

    wx, wy = oracle_lib.highway_map()
    m = ppamd.Map(wx, wy)
    prm = ppamd.default_params(noise_first_scene=0)
    scenes = ppamd.synth_device(m, S, seed=bench.parse([]).seed, first=0, device=0)
    res = ppamd.alloc_result(S, prm, xp="torch", device=torch.device("cuda", 0))
    ppamd.evaluate(m, scenes, prm, res, device=0)
    torch.cuda.synchronize()
    ref = ppamd.result_to_numpy(res)
    idx = np.load(tmp_path / "scene_index.npy")
    assert idx.dtype == np.float64 and len(idx) == (1000 if sampled else S)
    idx = idx.astype(np.int64)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([k + ".npy" for k in ref] + ["scene_index.npy"])
    for k, want in ref.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float64, k
        want = want[:, idx] if k in ("next_x", "next_y") else want[idx]
        assert np.array_equal(got, want.astype(np.float64), equal_nan=True), k
