"""Writes tests/golden/kitti_flow_tiny.png: a 3 x 4 KITTI-format flow map (16-bit RGB PNG) of
known samples, with the independent writer of tests/kitti_flow_np.py (zlib + struct, filter 0),
not with the project's encoder.  tests/test_kitti_flow_host.py holds the same table and checks
the project's decoder against it.

    python tests/golden/make_kitti_flow_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# (R, G, B): R is the x flow, G the y flow, B != 0 marks a valid pixel
TINY = np.array([
    # the range's ends, a valid pixel with zero flow, and (1, -2) px
    [(0, 0, 1), (32768, 32768, 1), (65535, 65535, 1), (32768 + 64, 32768 - 128, 1)],
    # an invalid pixel with samples, KITTI's all-zero invalid pixel, a plain one, +-1/64 px
    [(12345, 54321, 0), (0, 0, 0), (40000, 30000, 1), (32769, 32767, 1)],
    # samples whose two bytes differ (byte order), mixed ends, B other than 1
    [(256, 1, 1), (1, 256, 1), (65535, 0, 1), (0x1234, 0x5678, 0x9ABC)],
], np.uint16)

if __name__ == "__main__":
    import kitti_flow_np
    path = os.path.join(HERE, "kitti_flow_tiny.png")
    kitti_flow_np.write_png(path, TINY, filt=0)
    print(path, os.path.getsize(path), "bytes")
