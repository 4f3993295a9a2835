"""Golden vectors that pin super_resolution_amd/niqe.py (and through it csrc/hat_niqe.hip) to the reference's NIQE
(basicsr/metrics/niqe.py), loaded by file path together with the three files it imports from (utils/registry.py,
utils/color_util.py, utils/matlab_functions.py, metrics/metric_util.py); only `cv2` is a stub (convert_to='y' never calls it).
Needs scipy, as the reference does.

Run where the reference is (it does not travel):  python tests/golden/gen_golden_niqe.py <reference>/HAT/ESC/basicsr
Writes tests/golden/niqe.npz:
  mu_pris_param (36,), cov_pris_param (36,36), gaussian_window (7,7)   float64, the reference's niqe_pris_params.npz
  cases           JSON list of {name, crop_border}; per case NAME:
  NAME_img        (h,w,3) uint8 RGB   seeded image (the reference is fed the BGR view, as its callers do)
  NAME_score      float64   calculate_niqe(img, crop_border)              -- the float32 route; NaN for the all-flat image (there
                            the reference's pinv of a NaN covariance raises LinAlgError, recorded as NaN)
  NAME_score64    float64   niqe() of the same rounded Y plane as float64 -- what an fp64 evaluation of sigma would give
  NAME_feat       (nblocks, 36) float64   the per-block features of both scales, in the reference's block order
  strip_mscn      (96,192) float32   the first scale's normalised plane of case `strip`, put together from the blocks
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    for n in ("basicsr", "basicsr.utils", "basicsr.metrics", "cv2"):
        sys.modules[n] = types.ModuleType(n)
    load("basicsr.utils.registry", "utils/registry.py")
    sys.modules["basicsr.utils"].bgr2ycbcr = load("basicsr.utils.color_util", "utils/color_util.py").bgr2ycbcr
    load("basicsr.metrics.metric_util", "metrics/metric_util.py")
    load("basicsr.utils.matlab_functions", "utils/matlab_functions.py")
    return load("basicsr.metrics.niqe", "metrics/niqe.py")


def smooth(a, passes):
    """a cheap low-pass: `passes` 1-2-1 filters along both axes with edge replication (numpy only)."""
    for _ in range(passes):
        p = np.pad(a, 1, mode="edge")
        a = (p[:-2, 1:-1] + 2 * p[1:-1, 1:-1] + p[2:, 1:-1]) / 4
        p = np.pad(a, 1, mode="edge")
        a = (p[1:-1, :-2] + 2 * p[1:-1, 1:-1] + p[1:-1, 2:]) / 4
    return a


def textured(rng, h, w, passes, noise):
    """(h,w,3) uint8: smoothed noise plus noise, the three channels sharing the structure with their own noise on top."""
    base = smooth(rng.standard_normal((h, w)), passes)
    base = base / base.std()
    chans = [base + noise * rng.standard_normal((h, w)) for _ in range(3)]
    a = np.stack(chans, axis=2)
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * 255).astype(np.uint8)


def images():
    rng = np.random.default_rng(20262)
    out = [("mix", textured(rng, 192, 288, 6, 0.15), 0),
           ("strip", textured(rng, 96, 192, 3, 0.2), 0),
           ("crop", textured(rng, 200, 300, 10, 0.1), 4)]
    # A smooth gradient with little noise: sigma is small and the float32 cancellation in conv(img^2) - mu^2 decides it; the
    # float32 and the float64 route differ in the third digit.  At the SECOND scale such an image is as sensitive to one-ulp
    # differences of the half-size image, and the reference's imresize (Tensor.mv, summation order unspecified) and resize.py
    # (k ascending) differ by such ulps: over seeds 1000..1005 and noise 0.8..2.5 the host definition lands 2e-6 to 1e-2 from
    # the reference, all of it in the second scale's features (the first scale's agree to 1e-15 for every seed).  This seed
    # is one where the two imresize orders lead to the same fits, so the reference's score can be asked of the device.
    yy, xx = np.mgrid[0:192, 0:288]
    g = 60.0 + 120.0 * (0.6 * xx / 287.0 + 0.4 * yy / 191.0) + 10.0 * np.sin(xx / 37.0) * np.cos(yy / 29.0)
    g = g[..., None] + 1.8 * np.random.default_rng(1003).standard_normal((192, 288, 3))
    out.append(("smooth", np.clip(np.round(g), 0, 255).astype(np.uint8), 0))
    fb = textured(rng, 192, 288, 4, 0.2)
    fb[72:192, 72:216] = 131           # block (1, 1) and 24 pixels around it are flat (the 7x7 window and the half-size resize
    #                                    reach across block borders): its feature row has NaNs and nanmean / nancov drop it
    out.append(("flatblock", fb, 0))
    out.append(("flat", np.full((96, 192, 3), 90, dtype=np.uint8), 0))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    nq = load_reference(sys.argv[1])
    with np.load(os.path.join(sys.argv[1], "metrics", "niqe_pris_params.npz")) as z:
        data = {k: z[k].astype(np.float64) for k in ("mu_pris_param", "cov_pris_param", "gaussian_window")}
    rows, blocks, planes = [], [], []
    feature, niqe = nq.compute_feature, nq.niqe

    def record_feature(block):
        f = feature(block)
        rows.append(f)
        blocks.append(np.array(block))
        return f

    def record_niqe(img, *a, **k):
        planes.append(np.array(img))
        return niqe(img, *a, **k)
    nq.compute_feature, nq.niqe = record_feature, record_niqe
    cases = []
    warnings.simplefilter("ignore")
    for name, img, crop in images():
        del rows[:], blocks[:], planes[:]
        try:
            score = nq.calculate_niqe(img[:, :, ::-1], crop)
        except np.linalg.LinAlgError as e:      # the all-flat image: pinv of a NaN matrix
            print(name, "reference raises", repr(e), "-> recorded as NaN")
            score = float("nan")
        plane = planes[0]
        assert plane.dtype == np.float32
        nb = len(rows) // 2
        feat = np.concatenate([np.array(rows[:nb], dtype=np.float64), np.array(rows[nb:2 * nb], dtype=np.float64)], axis=1)
        if name == "strip":                     # blocks arrive column by column; one row of blocks here
            data["strip_mscn"] = np.concatenate(blocks[:nb], axis=1).astype(np.float32)
            assert data["strip_mscn"].shape == (96, 192) and blocks[0].dtype == np.float32
        try:
            score64 = niqe(plane.astype(np.float64), data["mu_pris_param"], data["cov_pris_param"], data["gaussian_window"])
        except np.linalg.LinAlgError:
            score64 = float("nan")
        data.update({f"{name}_img": img, f"{name}_score": np.float64(score), f"{name}_score64": np.float64(score64), f"{name}_feat": feat})
        cases.append({"name": name, "crop_border": crop})
        print(name, img.shape, "crop", crop, "blocks", nb, "score", score, "fp64 route", score64, "diff", abs(score - score64),
              "NaN rows", int(np.isnan(feat).any(axis=1).sum()))
    path = os.path.join(HERE, "niqe.npz")
    np.savez_compressed(path, cases=np.array(json.dumps(cases)), **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
