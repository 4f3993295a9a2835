"""Golden vectors that pin super_resolution_amd/yuv.py to the reference's colour conversion: `rgb2ycbcr` and `ycbcr2rgb` of
basicsr/utils/color_util.py (BT.601, 16-235), loaded by file path (the file needs only numpy and torch).

Run where the reference is (it does not travel):  python tests/golden/gen_golden_yuv.py <reference>/HAT/ESC/basicsr/utils/color_util.py
Writes tests/golden/ycbcr_bt601.npz:
  ycc        (N,3) uint8   seeded YCbCr triples, with the corners and every byte value in each column
  rgb_ref    (N,3) float32 ycbcr2rgb(float32(ycc) / 255)                    (not clipped)
  rgb        (96,3) float32 seeded RGB in [0, 1], with the corners
  ycc_ref    (96,3) float32 rgb2ycbcr(rgb)                                   ([0, 1] units: Y, Cb, Cr over 255)
The test evaluates the same constants in fp64 itself, to check that the reference alone stays inside the bars it sets for yuv.py.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_color_util", path)
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    rng = np.random.default_rng(20260)
    n = 288
    ycc = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    ycc[:256] = np.arange(256, dtype=np.uint8)[:, None]                      # every byte value in every column
    ycc[256:264] = [[16, 128, 128], [235, 128, 128], [16, 16, 16], [235, 240, 240], [16, 128, 16], [235, 128, 240], [0, 0, 0], [255, 255, 255]]
    rgb_ref = cu.ycbcr2rgb(ycc.astype(np.float32) / np.float32(255.0))
    M = np.array([[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]])
    rgb_exact = (ycc.astype(np.float64) @ M * 255.0 + np.array([-222.921, 135.576, -276.836])) / 255.0
    rgb = rng.random((96, 3), dtype=np.float32)
    rgb[:8] = [[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [1, 1, 0], [0, 1, 1]]
    ycc_ref = cu.rgb2ycbcr(rgb)
    K = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])
    ycc_exact = rgb.astype(np.float64) @ K + np.array([16.0, 128.0, 128.0])
    assert rgb_ref.dtype == np.float32 and ycc_ref.dtype == np.float32
    out = os.path.join(HERE, "ycbcr_bt601.npz")
    np.savez_compressed(out, ycc=ycc, rgb_ref=rgb_ref, rgb=rgb, ycc_ref=ycc_ref)
    print(out, os.path.getsize(out), "bytes;",
          "reference vs fp64: in", float(np.abs(np.clip(rgb_ref, 0, 1) - np.clip(rgb_exact, 0, 1)).max()),
          "out", float(np.abs(255.0 * ycc_ref.astype(np.float64) - ycc_exact).max()))


if __name__ == "__main__":
    main()
