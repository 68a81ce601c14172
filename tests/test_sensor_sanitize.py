"""The sensor model's shared arithmetic (csrc/pp_sensor.h: what k_sense and pp_sense_frame_host evaluate)
under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone host program, the way
tests/test_world_sanitize.py runs the other world stages' programs.
`make -C carnd-path-planning-project_amd sanitize-sensor` builds tests/sanitize/sensor_host.cpp over
tests/sanitize/world_fixture.h with -fsanitize=address,undefined -fno-sanitize-recover=all. The truth and
the sensor state are vectors of exactly the documented sizes:
  sensor_host       the hand-made scene (the middle car of a line hides the far one) with every output
                    checked; 300 seeded frames (64 scenes of 100 cars with every row in use, car_stride 1
                    to 100, ids and frame numbers up to 2^31 - 1, NaN and infinite positions, a car at the
                    ego's position, occlusion on and off, dropout 0, 0.3 and 1): fates against the counts,
                    compaction in truth order, the identity sensor's rows, rows beyond the count untouched
Any sanitizer report aborts the program; the test requires a clean exit and the lines its scenarios
print. The program links its sanitizer runtime itself; nothing is loaded into Python. CPU only."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "carnd-path-planning-project_amd")
LINES = ["sensor: hand-made case", "random frames"]


def test_sensor_host_code_sanitizer_clean():
    assert shutil.which("g++") is not None, "no host compiler: the sanitizer run cannot be skipped silently"
    r = subprocess.run(["make", "-C", PKG, "-s", "sanitize-sensor"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "asan", "sensor_host")], capture_output=True, text=True,
                       timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("clean")
    for line in LINES:
        assert line in r.stdout, line
