"""Closed-loop rollout: the planner's cross-frame state — the reference's
persistent std::map car table with stale entries (src/main.cpp:1194, 1325-1350) and target_lane
(:1195) — driven by the simulator shim of include/pp.h (pp_rollout).

Pinning: tests/golden/rollout_golden.npz holds 600-frame replays made by the reference's own frame
code (tests/golden/make_rollout_golden.py); the C restatement must reproduce them bit for bit; the
HIP rollout must match them within 1e-6 m, and match the restatement frame by frame."""
import numpy as np
import pytest

import oracle_lib
from oracle_lib import ppamd
from world_lib import many_car_traffic

TOL = 1e-6
G = np.load(oracle_lib.GOLDEN + "/rollout_golden.npz")
VARIANTS = ["r120", "rinf"]
LOG_KEYS = ["ego_x", "ego_y", "ego_speed_mph", "target_lane", "n_out", "n_cars"]


def golden_state(v):
    sc = {k[len(v) + 7:]: np.array(G[k]) for k in G.files if k.startswith(f"{v}_scene_")}
    tr = {k[len(v) + 9:]: np.array(G[k]) for k in G.files if k.startswith(f"{v}_traffic_")}
    tr["n_cars"] = int(tr["n_cars"])
    return sc, tr


@pytest.fixture(scope="module")
def cpu():
    wx, wy = oracle_lib.highway_map()
    return {"m": ppamd.Map(wx, wy), "wx": wx, "wy": wy, "olib": oracle_lib.load_oracle(),
            "rlib": oracle_lib.load_ref()}


@pytest.mark.parametrize("v", VARIANTS)
def test_restatement_reproduces_reference_replay(cpu, v):
    sc, tr = golden_state(v)
    F = int(G["frames"])
    lg = oracle_lib.oracle_rollout(cpu["olib"], cpu["wx"], cpu["wy"], sc, tr, ppamd.default_params(n_speeds=1),
                                   F, int(G["consume"]), float(G[f"{v}_range"]))
    for k in LOG_KEYS:
        np.testing.assert_array_equal(lg[k], G[f"{v}_ref_{k}"], err_msg=k)
    pf = int(G["plan_frames"])
    np.testing.assert_array_equal(lg["plan_x"][:pf], G[f"{v}_ref_plan_x"])
    np.testing.assert_array_equal(lg["plan_y"][:pf], G[f"{v}_ref_plan_y"])
    if v == "r120":
        # cars leave the sensor range: the table keeps stale entries the planner still uses
        assert (sc["tab_valid"].sum(0) > sc["n_cars"]).any()


def test_start_state_matches_synthetic_scenes(cpu):
    """pp_synth_traffic_host writes the same scenes as pp_synth_scenes_host, and every car's
    traffic state reproduces its reported position."""
    sc, tr = ppamd.synth_traffic_host(cpu["m"], 64, seed=99)
    ref = ppamd.synth_host(cpu["m"], 64, seed=99)
    for k in ref:
        np.testing.assert_array_equal(sc[k], ref[k], err_msg=k)
    assert tr["n_cars"] == 12 and not sc["tab_valid"].any()


@pytest.mark.skipif(oracle_lib.load_ref() is None, reason="oracle/_ref not built (no reference here)")
@pytest.mark.parametrize("seed,consume,rng", [(3, 1, 80.0), (4, 5, 200.0), (5, 3, 60.0)])
def test_restatement_vs_reference_live(cpu, seed, consume, rng):
    """Fresh seeds, other consume counts and ranges, against the reference build itself."""
    sc, tr = ppamd.synth_traffic_host(cpu["m"], 6, seed=seed)
    a, b = oracle_lib.copy_state(sc, tr), oracle_lib.copy_state(sc, tr)
    lo = oracle_lib.oracle_rollout(cpu["olib"], cpu["wx"], cpu["wy"], *a, ppamd.default_params(n_speeds=1),
                                   300, consume, rng)
    lr = oracle_lib.ref_rollout(cpu["rlib"], cpu["wx"], cpu["wy"], *b, 300, consume, rng)
    for k in LOG_KEYS + ["plan_x", "plan_y"]:
        np.testing.assert_array_equal(lo[k], lr[k], err_msg=k)


@pytest.mark.skipif(oracle_lib.load_ref() is None, reason="oracle/_ref not built (no reference here)")
def test_restatement_vs_reference_100_cars(cpu):
    """100 cars in the loop (more than the former 64-car limit): the restatement equals the
    reference's own frame code (std::map car table) bit for bit over 300 frames."""
    sc, tr = many_car_traffic(cpu["m"], 4, 21)
    a, b = oracle_lib.copy_state(sc, tr), oracle_lib.copy_state(sc, tr)
    lo = oracle_lib.oracle_rollout(cpu["olib"], cpu["wx"], cpu["wy"], *a, ppamd.default_params(n_speeds=1),
                                   300, 3, 1e5)
    lr = oracle_lib.ref_rollout(cpu["rlib"], cpu["wx"], cpu["wy"], *b, 300, 3, 1e5)
    for k in LOG_KEYS + ["plan_x", "plan_y"]:
        np.testing.assert_array_equal(lo[k], lr[k], err_msg=k)
    assert lr["n_cars"].max() > 64, lr["n_cars"].max()


@pytest.mark.gpu
class TestRolloutGPU:
    @pytest.fixture(scope="class")
    def env(self):
        import torch
        wx, wy = oracle_lib.highway_map()
        return {"torch": torch, "m": ppamd.Map(wx, wy), "wx": wx, "wy": wy,
                "olib": oracle_lib.load_oracle(), "dev": torch.device("cuda", 0)}

    def upload(self, env, sc, tr):
        t = env["torch"]
        d = {k: t.from_numpy(np.ascontiguousarray(v)).to(env["dev"]) for k, v in sc.items()}
        g = {k: (t.from_numpy(np.ascontiguousarray(v)).to(env["dev"]) if isinstance(v, np.ndarray) else v)
             for k, v in tr.items()}
        return d, g

    @pytest.mark.parametrize("v", VARIANTS)
    def test_gpu_replay_matches_reference(self, env, v):
        sc, tr = golden_state(v)
        d, g = self.upload(env, sc, tr)
        F, S = int(G["frames"]), sc["ego_x"].shape[0]
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
        lg = ppamd.alloc_log(F, S, 50, xp="torch", device=env["dev"])
        ppamd.rollout(env["m"], d, g, prm, res, F, int(G["consume"]), float(G[f"{v}_range"]), lg)
        env["torch"].cuda.synchronize()
        got = {k: x.cpu().numpy() for k, x in lg.items()}
        for k in ["target_lane", "n_out", "n_cars"]:
            np.testing.assert_array_equal(got[k], G[f"{v}_ref_{k}"], err_msg=k)
        for k in ["ego_x", "ego_y"]:
            e = np.abs(got[k] - G[f"{v}_ref_{k}"]).max()
            assert e <= TOL, (k, e)
        pf = int(G["plan_frames"])
        for k in ["plan_x", "plan_y"]:
            e = np.abs(got[k][:pf] - G[f"{v}_ref_{k}"]).max()
            assert e <= TOL, (k, e)
        print(f"{v}: {S} scenes x {F} frames, max |d ego| "
              f"{max(np.abs(got['ego_x'] - G[f'{v}_ref_ego_x']).max(), np.abs(got['ego_y'] - G[f'{v}_ref_ego_y']).max()):.2e} m")

    def test_frame_by_frame_vs_restatement(self, env):
        """Every frame of a GPU episode, re-run by the restatement from the GPU's own state:
        plan within 1e-6 m, the car table and traffic identical, the next telemetry identical
        (yaw within 1e-9 deg: the simulator's atan2 is the device library's)."""
        t = env["torch"]
        S, F = 384, 40
        d, g = ppamd.synth_traffic(env["m"], S, seed=11, device=0)
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
        for f in range(F):
            sc = {k: x.cpu().numpy() for k, x in d.items()}
            tr = {k: (x.cpu().numpy() if isinstance(x, t.Tensor) else x) for k, x in g.items()}
            lo = oracle_lib.oracle_rollout(env["olib"], env["wx"], env["wy"], sc, tr, prm, 1, 3, 100.0)
            lg = ppamd.alloc_log(1, S, 50, xp="torch", device=env["dev"])
            ppamd.rollout(env["m"], d, g, prm, res, 1, 3, 100.0, lg)
            t.cuda.synchronize()
            got = {k: x.cpu().numpy() for k, x in lg.items()}
            np.testing.assert_array_equal(got["target_lane"], lo["target_lane"])
            np.testing.assert_array_equal(got["n_out"], lo["n_out"])
            for k in ["plan_x", "plan_y"]:
                assert np.abs(got[k] - lo[k]).max() <= TOL, (f, k)
            new = {k: x.cpu().numpy() for k, x in d.items()}
            for k in new:
                if k == "ego_yaw_deg":
                    np.testing.assert_allclose(new[k], sc[k], rtol=0, atol=1e-9)
                elif new[k].dtype.kind == "f":
                    assert np.abs(new[k] - sc[k]).max() <= TOL, (f, k)
                else:
                    np.testing.assert_array_equal(new[k], sc[k], err_msg=f"{f} {k}")
            for k in ["seg", "t"]:
                np.testing.assert_array_equal(g[k].cpu().numpy(), tr[k])

    def test_plan_frame_episode_keeps_car_table(self, env):
        """pp_plan_frame (the onMessage replacement) over consecutive frames of one episode with
        cars leaving the sensor range: its persistent table must reproduce the restatement's
        closed loop (stale entries included) frame after frame."""
        sc, tr = golden_state("r120")
        one = {k: np.ascontiguousarray(v[..., :1]) for k, v in sc.items()}
        tone = {k: (np.ascontiguousarray(v[..., :1]) if isinstance(v, np.ndarray) else v) for k, v in tr.items()}
        prm = ppamd.default_params(n_speeds=1)
        ppamd.plan_reset(env["m"])
        stale_frames = 0
        for f in range(150):
            tel = {k: v.copy() for k, v in one.items()}
            lg = oracle_lib.oracle_rollout(env["olib"], env["wx"], env["wy"], one, tone, prm, 1, 3, 120.0)
            nc = int(tel["n_cars"][0])
            cars = [(int(tel["car_id"][j, 0]), tel["car_x"][j, 0], tel["car_y"][j, 0], tel["car_vx"][j, 0],
                     tel["car_vy"][j, 0]) for j in range(nc)]
            npv = int(tel["n_prev"][0])
            nx, ny, tl = ppamd.plan_frame(env["m"], tel["ego_x"][0], tel["ego_y"][0], tel["ego_yaw_deg"][0],
                                          tel["ego_speed_mph"][0], tel["prev_x"][:min(npv, 10), 0],
                                          tel["prev_y"][:min(npv, 10), 0], cars,
                                          target_lane=int(tel["prev_target_lane"][0]))
            n = int(lg["n_out"][0, 0])
            assert len(nx) == n and tl == int(lg["target_lane"][0, 0]), f
            e = max(np.abs(nx - lg["plan_x"][0, :n, 0]).max(initial=0), np.abs(ny - lg["plan_y"][0, :n, 0]).max(initial=0))
            assert e <= TOL, (f, e)
            stale_frames += int(one["tab_valid"][:, 0].sum() > nc)
        assert stale_frames > 0

    def test_large_batch_rollout(self, env):
        """65,536 scenes x 60 frames: finite, lanes valid, plans full length."""
        t = env["torch"]
        S, F = 65536, 60
        d, g = ppamd.synth_traffic(env["m"], S, seed=12, device=0)
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
        lg = ppamd.alloc_log(F, S, 50, xp="torch", device=env["dev"], plans=False)
        ppamd.rollout(env["m"], d, g, prm, res, F, 3, 300.0, lg)
        t.cuda.synchronize()
        tl = lg["target_lane"].cpu().numpy()
        assert ((tl >= 0) & (tl <= 2)).all()
        assert np.isfinite(lg["ego_x"].cpu().numpy()).all()
        assert (lg["n_out"].cpu().numpy()[1:] >= 40).mean() > 0.99

    @pytest.mark.skipif(oracle_lib.load_ref() is None, reason="oracle/_ref not built")
    def test_gpu_100_cars_vs_reference(self, env):
        """100 cars (100 sensor_fusion rows every frame, a 100-slot car table) in the HIP closed
        loop against the reference's own frame code over 300 frames: target lanes, point counts
        and car counts exact, ego track and plans within 1e-6 m."""
        sc, tr = many_car_traffic(env["m"], 64, 23)
        a = oracle_lib.copy_state(sc, tr)
        d, g = self.upload(env, sc, tr)
        F, S = 300, 64
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
        lg = ppamd.alloc_log(F, S, 50, xp="torch", device=env["dev"])
        ppamd.rollout(env["m"], d, g, prm, res, F, 3, 1e5, lg)
        env["torch"].cuda.synchronize()
        got = {k: x.cpu().numpy() for k, x in lg.items()}
        lr = oracle_lib.ref_rollout(oracle_lib.load_ref(), env["wx"], env["wy"], *a, F, 3, 1e5)
        for k in ["target_lane", "n_out", "n_cars"]:
            np.testing.assert_array_equal(got[k], lr[k], err_msg=k)
        e = 0.0
        for k in ["ego_x", "ego_y", "plan_x", "plan_y"]:
            e = max(e, float(np.abs(got[k] - lr[k]).max()))
        assert e <= TOL, e
        assert lr["n_cars"].max() > 64
        print(f"100 cars: {S} scenes x {F} frames, up to {lr['n_cars'].max()} reported, max |d| {e:.2e} m")

    def test_gpu_100_dense_cars_frame_by_frame(self, env):
        """Dense 100-car traffic (cars drive through each other and the ego): every frame of a GPU
        episode re-run by the restatement from the GPU's own state (the reference-pinned
        restatement, tests/test_rollout.py::test_restatement_vs_reference_100_cars): target lanes
        and point counts exact, plans within 1e-6 m, the car table identical. (A free-running
        comparison of such traffic is chaotic: an ulp in a fed-back point meets near-ties of the
        collision and braking rules.)"""
        t = env["torch"]
        S, F = 64, 150
        sc, tr = many_car_traffic(env["m"], S, 23, dense=True)
        d, g = self.upload(env, sc, tr)
        prm = ppamd.default_params(n_speeds=1)
        res = ppamd.alloc_result(S, prm, xp="torch", device=env["dev"])
        worst, rows = 0.0, 0
        for f in range(F):
            hs = {k: x.cpu().numpy() for k, x in d.items()}
            ht = {k: (x.cpu().numpy() if isinstance(x, t.Tensor) else x) for k, x in g.items()}
            lo = oracle_lib.oracle_rollout(env["olib"], env["wx"], env["wy"], hs, ht, prm, 1, 3, 400.0)
            lg = ppamd.alloc_log(1, S, 50, xp="torch", device=env["dev"])
            ppamd.rollout(env["m"], d, g, prm, res, 1, 3, 400.0, lg)
            t.cuda.synchronize()
            got = {k: x.cpu().numpy() for k, x in lg.items()}
            np.testing.assert_array_equal(got["target_lane"], lo["target_lane"], err_msg=str(f))
            np.testing.assert_array_equal(got["n_out"], lo["n_out"], err_msg=str(f))
            for k in ["plan_x", "plan_y"]:
                worst = max(worst, float(np.abs(got[k] - lo[k]).max()))
            new = {k: x.cpu().numpy() for k, x in d.items()}
            for k in ("tab_valid", "tab_lane", "n_cars", "car_id"):
                np.testing.assert_array_equal(new[k], hs[k], err_msg=f"{f} {k}")
            rows = max(rows, int(new["n_cars"].max()))
        assert worst <= TOL, worst
        assert rows > 64, rows
        print(f"dense 100 cars: {S} scenes x {F} frames, up to {rows} rows, max |dxy| {worst:.2e} m")
