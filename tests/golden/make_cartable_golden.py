"""Generates tests/golden/cartable_golden.npz: 12 closed-loop episodes of 25 frames (cartable_lib
record_episodes), each planned by its own REFERENCE session — oracle/_ref/libppref.so, the classes of
src/main.cpp with main()'s persistent std::map car table and target_lane. The episodes' car ids are
sparse, negative, -1, INT32_MIN and 2^31 - 2 among them (3 to 30 cars); the sensor ranges leave
stale entries and some cars leave the road, so entries are erased.

Stored: per episode and frame the telemetry (ego, the first 10 previous points and their count, the
sensor_fusion rows in the order sent, the target lane going in) and the session's outputs (next
points, their count, the target lane, the number of entries in its map). Recorded inputs and results
only. The C restatement in car-table mode (one batch of 12 scenes over 33 slots, a Python dict per
scene as the map) is asserted equal to the sessions on the same record before anything is written
(tests/test_cartable_shapes.py runs the same check from the file).

Run from the repo root (needs oracle/_ref built by `make -C oracle`):
    python tests/golden/make_cartable_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cartable_lib  # noqa: E402
import oracle_lib  # noqa: E402
from oracle_lib import ppamd  # noqa: E402


def main():
    wx, wy = oracle_lib.highway_map()
    rlib = oracle_lib.load_ref_session()
    assert rlib is not None, "oracle/_ref/libppref.so not built"
    rec = cartable_lib.record_episodes(ppamd.Map(wx, wy), wx, wy, rlib)
    census = cartable_lib.check_oracle_table_batch(oracle_lib.load_oracle(), wx, wy, rec)
    path = os.path.join(HERE, "cartable_golden.npz")
    np.savez_compressed(path, **rec)
    print(f"{rec['n_rows'].shape[0]} episodes x {rec['n_rows'].shape[1]} frames, reference == restatement; "
          f"rows/frame {rec['n_rows'].min()}..{rec['n_rows'].max()}, census {census}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
