"""Writes tests/golden/pil_bicubic.npz: for every case of tests/arb_eval_cases.py the seeded input (`<name>.in`) and what Pillow's
8-bit bicubic `Image.resize` makes of it (`<name>.out`).  Inputs and outputs only; needs Pillow.

    python tests/golden/gen_golden_pil_bicubic.py
"""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arb_eval_cases as cases  # noqa: E402


def main():
    out = {}
    for name, (_, (oh, ow), _) in cases.RESIZE_CASES.items():
        src = cases.source(name)
        out[name + ".in"] = src
        out[name + ".out"] = np.asarray(Image.fromarray(src, "RGB").resize((ow, oh), Image.BICUBIC), dtype=np.uint8)
    np.savez_compressed(cases.GOLDEN, **out)
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
