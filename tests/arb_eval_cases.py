"""The resize cases of the ESC-LTE benchmark loop's tests (test_arb_eval_cpu.py, test_gpu_arb_eval.py) and of the generator of
tests/golden/pil_bicubic.npz (tests/golden/gen_golden_pil_bicubic.py): seeded inputs, so the golden file, a live Pillow and the
device all see the same bytes."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_bicubic.npz")

# name -> ((h, w), (oh, ow), fill): fill None is seeded noise, a number is a constant image (a rounding-constant or clip error that
# noise hides shows on 255 and on 0)
RESIZE_CASES = {
    "half": ((37, 53), (18, 26), None),
    "third": ((37, 53), (12, 17), None),
    "quarter": ((37, 53), (9, 13), None),
    "unequal": ((37, 53), (24, 35), None),
    "enlarge": ((37, 53), (48, 69), None),
    "div30": ((64, 95), (2, 3), None),          # / 32 and / 31.7: 129 and 127 table columns, more than the 121 of x30
    "to_one": ((9, 9), (1, 1), None),
    "white_third": ((37, 53), (12, 17), 255),
    "white_enlarge": ((37, 53), (48, 69), 255),
    "black_third": ((37, 53), (12, 17), 0),
}


def source(name: str) -> np.ndarray:
    (h, w), _, fill = RESIZE_CASES[name]
    if fill is not None:
        return np.full((h, w, 3), fill, dtype=np.uint8)
    return np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, (h, w, 3), dtype=np.uint8)


def noise(key: str, shape, lo=0, hi=256) -> np.ndarray:
    return np.random.default_rng(zlib.crc32(key.encode())).integers(lo, hi, shape, dtype=np.uint8)


def psnr_pair(h=40, w=56, ph=40, pw=56):
    """-> (pred float32 (3,ph,pw), gt (h,w,3) uint8): the ground truth plus noise, stretched so that it leaves [0, 1] on both sides
    (the clamp counts)."""
    gt = noise(f"arb.gt{h}x{w}", (h, w, 3))
    base = np.full((3, ph, pw), 0.5, np.float32)
    base[:, :h, :w] = gt.transpose(2, 0, 1).astype(np.float32) / 255
    rng = np.random.default_rng(zlib.crc32(f"arb.pred{ph}x{pw}".encode()))
    pred = (base + rng.normal(0, 0.08, (3, ph, pw))).astype(np.float32) * np.float32(1.3) - np.float32(0.15)
    assert (pred < 0).any() and (pred > 1).any()
    return pred, gt


def golden() -> dict:
    return dict(np.load(GOLDEN))
