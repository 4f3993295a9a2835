"""What tests/test_niqe_cpu.py and tests/test_gpu_niqe.py share: the golden file, the extra seeded frames and the bars.

The bars are measured on the CPU over the golden images (test_niqe_cpu.test_bars_are_measured recomputes them) between the
host definition as it is (block sums added in float32, numpy's pairwise order: the reference's own arithmetic) and the host
definition with the same float32 values added in fp64 (what the device does):
  largest |score - score(fp64 block sums)|                      1.21e-6   (image `mix`; scores 9.8 to 18.4)
  largest relative difference of any of the 21 sums             1.33e-7   (image `smooth`)
SCORE_BAR and SUM_BAR are 10 x those: headroom for another fp64 reduction order and a rare one-ulp difference in a rounding of
mu.  Neither comes from what a kernel returns.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niqe.npz")
MEASURED_SCORE, MEASURED_SUM = 1.21e-6, 1.33e-7
SCORE_BAR, SUM_BAR = 10 * MEASURED_SCORE, 10 * MEASURED_SUM
COUNT_COLUMNS = [5 * m + q for m in range(5) for q in (0, 1)]     # compared exactly (all ten, which covers the issue's four)
SUM_COLUMNS = [5 * m + q for m in range(5) for q in (2, 3, 4)]     # compared at SUM_BAR, relative


def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g["cases"] = json.loads(str(g["cases"]))
    g["pris"] = {"mu_pris_param": g["mu_pris_param"], "cov_pris_param": g["cov_pris_param"]}
    return g


def checkerboard_frame():
    """192 x 288: a checkerboard of the levels 0 and 255 in the top-left 96 x 96 block, seeded noise in the other five.  There
    conv(img^2) - mu^2 is largest in float32 while mu sits between two levels: a kernel that rounded mu late would show."""
    f = np.random.default_rng(4242).integers(0, 256, (192, 288, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:96, 0:96]
    f[:96, :96] = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]
    return f


def noise_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
