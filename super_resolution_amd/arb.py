"""Arbitrary-scale super-resolution of a folder of images with ESC-LTE, the reference's ESC/esc_arb/inference.py:51-95 on the MI355X.

    python -m super_resolution_amd.arb --model ckpt.pth --input-path DIR --output-path DIR (--scale S | --size H W) [--is-lr]
                                       [--scale-max 4] [--compute-dtype bf16|fp32]

`--model` is the reference's checkpoint ({'model': {'name': 'lte', 'args': ..., 'sd': ...}}, `ESCLTE.from_checkpoint`).  With
`--is-lr` every image is the low-resolution input and the output is `int(H * S)` x `int(W * S)` (S need not be an integer, unlike
the reference's), or exactly `--size`.  Without it the image is the ground truth: it is first shrunk on the host by the integer S
with PIL's bicubic filter, exactly as the reference's `resize_fn` does (ToPILImage's `mul(255).byte()`, `Image.resize`, ToTensor's
division by 255), and brought back to its own size; `--size` or a fractional S is refused there.  The output is clamped to [0, 1]
and converted as the reference's ToPILImage converts it (x255, truncated), then written with the harness's PIL writer."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from .data import _EXT, read_image, write_image


def shrink_like_the_reference(img: torch.Tensor, size) -> torch.Tensor:
    """inference.py:16-19: img (3,H,W) float in [0, 1] -> (3,h,w), through an 8-bit PIL image and PIL's bicubic resize."""
    from PIL import Image
    u8 = img.mul(255).byte().permute(1, 2, 0).contiguous().numpy()
    small = Image.fromarray(u8, "RGB").resize((int(size[1]), int(size[0])), Image.BICUBIC)
    return torch.from_numpy(np.asarray(small, dtype=np.uint8).copy()).permute(2, 0, 1).to(torch.float32).div(255)


def plan_sizes(H: int, W: int, *, scale, size, is_lr: bool):
    """-> ((h_in, w_in) of the network's input or None when it is the image itself, (h, w) of the output)."""
    if (scale is None) == (size is None):
        raise ValueError("give exactly one of --scale and --size")
    if is_lr:
        return None, ((int(H * scale), int(W * scale)) if size is None else (int(size[0]), int(size[1])))
    if size is not None or int(scale) != scale or scale < 1:
        raise ValueError("without --is-lr the image is shrunk by an integer --scale first, as the reference does (h // scale, w // scale): "
                         "--size and a fractional --scale need --is-lr")
    s = int(scale)
    if H // s < 1 or W // s < 1:
        raise ValueError(f"a {H}x{W} image cannot be shrunk by {s}")
    return (H // s, W // s), (H, W)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m super_resolution_amd.arb", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True)
    ap.add_argument("--input-path", "--input_path", dest="input_path", required=True)
    ap.add_argument("--output-path", "--output_path", dest="output_path", required=True)
    ap.add_argument("--scale", type=float, default=None)
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"))
    ap.add_argument("--is-lr", "--is_lr", dest="is_lr", action="store_true")
    ap.add_argument("--scale-max", type=float, default=4)
    ap.add_argument("--compute-dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    try:
        plan_sizes(64, 64, scale=args.scale, size=args.size, is_lr=args.is_lr)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("super_resolution_amd.arb needs a GPU: the MI355X HIP path is the only path (no CPU fallback)")
    from .archs.esc_lte_arch import ESCLTE
    dev = torch.device("cuda", args.gpu)
    net = ESCLTE.from_checkpoint(torch.load(args.model, map_location="cpu", weights_only=True), compute_dtype=args.compute_dtype).to(dev)
    names = sorted(f for f in os.listdir(args.input_path) if f.lower().endswith(_EXT))
    os.makedirs(args.output_path, exist_ok=True)
    for name in names:
        img = read_image(os.path.join(args.input_path, name))
        shrink, (h, w) = plan_sizes(img.shape[-2], img.shape[-1], scale=args.scale, size=args.size, is_lr=args.is_lr)
        if shrink is not None:
            img = shrink_like_the_reference(img, shrink)
        y = net.upscale(img[None].to(dev), size=(h, w), scale_max=args.scale_max)[0]
        out = y.clamp(0, 1).mul(255).byte().permute(1, 2, 0).contiguous().cpu().numpy()   # ToPILImage's conversion (inference.py:73-74)
        write_image(out, os.path.join(args.output_path, name))
        print(f"{name}: {tuple(img.shape[-2:])} -> {(h, w)}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
