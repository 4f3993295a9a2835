"""Golden vectors that pin super_resolution_amd/resize.py to the reference's `imresize` and `calculate_weights_indices`
(basicsr/utils/matlab_functions.py:16-178), loaded by file path (the file needs only numpy and torch).

Run where the reference is (it does not travel):  python tests/golden/gen_golden_resize.py <reference>/HAT/ESC/basicsr/utils/matlab_functions.py
Writes tests/golden/imresize.npz.  `cases` is a JSON list of {name, h, w, scale, antialiasing}; per case NAME:
  NAME_img        (h,w,3) uint8    seeded image, with flat, black and white patches
  NAME_out        (oh,ow,3) float32  imresize(float32(img) / 255, scale, antialiasing)     (HWC, unrounded, unclamped)
  NAME_wh, NAME_ww  float32 (out_len,P)  the reference's weights per axis
  NAME_ih, NAME_iw  int32 (out_len,P)    the reference's indices INTO THE AUGMENTED image (symmetric copy in front)
  NAME_sym        int32 (4,)       sym_len_hs, sym_len_he, sym_len_ws, sym_len_we
"""
from __future__ import annotations

import importlib.util
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("x4", 48, 68, 1 / 4, True), ("x3", 48, 66, 1 / 3, True), ("x2", 50, 70, 1 / 2, True), ("s075", 37, 53, 0.75, True),
         ("s03", 50, 70, 0.3, True), ("up2", 20, 28, 2.0, True), ("up3", 19, 23, 3.0, True), ("tiny", 9, 9, 1 / 4, True),
         ("x2_noaa", 50, 70, 1 / 2, False)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("ref_matlab_functions", sys.argv[1])
    mf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mf)
    rng = np.random.default_rng(20261)
    data, cases = {}, []
    for name, h, w, scale, aa in CASES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[: h // 4, : w // 4] = 255                       # white next to noise: the overshoot
        img[h // 2: h // 2 + 3, w // 2:] = 0
        img[-(h // 5):, -(w // 5):] = 77                      # flat: weights that sum to one give it back
        out = mf.imresize(img.astype(np.float32) / np.float32(255.0), scale, antialiasing=aa)
        oh, ow = math.ceil(h * scale), math.ceil(w * scale)
        assert out.shape == (oh, ow, 3) and out.dtype == np.float32
        wh, ih, hs, he = mf.calculate_weights_indices(h, oh, scale, "cubic", 4, aa)
        ww, iw, ws, we = mf.calculate_weights_indices(w, ow, scale, "cubic", 4, aa)
        data.update({f"{name}_img": img, f"{name}_out": out, f"{name}_wh": wh.numpy(), f"{name}_ww": ww.numpy(),
                     f"{name}_ih": ih.numpy().astype(np.int32), f"{name}_iw": iw.numpy().astype(np.int32),
                     f"{name}_sym": np.array([hs, he, ws, we], dtype=np.int32)})
        cases.append({"name": name, "h": h, "w": w, "scale": scale, "antialiasing": aa})
        print(name, f"{h}x{w} -> {oh}x{ow}", "P", wh.shape[1], ww.shape[1], "sym", hs, he, ws, we, "range", float(out.min()), float(out.max()))
    path = os.path.join(HERE, "imresize.npz")
    np.savez_compressed(path, cases=np.array(json.dumps(cases)), **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
