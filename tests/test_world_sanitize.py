"""The world stages' shared arithmetic under AddressSanitizer + UndefinedBehaviorSanitizer, as
stand-alone host programs: csrc/pp_judge.h, pp_follow.h, pp_lanechange.h and pp_episode.h, each the
one function behind a kernel (k_judge, k_follow, k_lane_change, k_synth_episode) and its host twin.
`make -C carnd-path-planning-project_amd sanitize-judge` (-follow, -lane-change, -episode) builds
tests/sanitize/<program>.cpp over tests/sanitize/world_fixture.h with -fsanitize=address,undefined
-fno-sanitize-recover=all. Every program holds every array in a vector of exactly the documented
size:
  judge_host        the 90-step ring-wrap drive grouped and split into single steps (identical bits),
                    seeded random frames (any n_out against any consume, 0 to 20 cars, every valid
                    window pair, restarted episodes)
  follow_host       a platoon behind the ego by hand, a free road whose speeds keep their bits, seeded
                    random frames (0 to 20 cars, parked and coinciding ones, the ego on, between and far
                    from the lanes, random valid configurations, restarted episodes)
  lane_change_host  the overtake frame by hand (the change, the kept position, the offset's way home),
                    seeded random episodes (as follow_host's, and calls before any follow update)
  episode_host      the default start's gaps, states and first follow update, that shards concatenate,
                    seeded random configurations (0 to 20 cars, egos at rest, parked cars, no table,
                    no states)
Any sanitizer report aborts a program; the test requires a clean exit and the lines its scenarios
print. The programs link their sanitizer runtime themselves; nothing is loaded into Python. CPU only."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "carnd-path-planning-project_amd")

# program: (make target, what its stdout must hold)
PROGRAMS = {
    "judge_host": ("sanitize-judge", ["judge: ring wrap and split calls, 90 steps", "random frames"]),
    "follow_host": ("sanitize-follow", ["follow: platoon of three", "free road", "random frames"]),
    "lane_change_host": ("sanitize-lane-change", ["lane change: overtake by hand", "random frames"]),
    "episode_host": ("sanitize-episode", ["episode: defaults", "one follow update", "shards concatenate",
                                          "random configurations"]),
}


@pytest.mark.parametrize("program", PROGRAMS)
def test_host_code_sanitizer_clean(program):
    target, lines = PROGRAMS[program]
    assert shutil.which("g++") is not None, "no host compiler: the sanitizer run cannot be skipped silently"
    r = subprocess.run(["make", "-C", PKG, "-s", target], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "asan", program)], capture_output=True, text=True, timeout=300,
                       env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("clean")
    for line in lines:
        assert line in r.stdout, line
