"""tools/arb_eval_path.py — what one image of the ESC-LTE benchmark loop costs: the device path (ESCLTE.score_gt_u8) against the host
composition it replaces, on a 1020x1356 ground truth at x2, x4 and x12.

    python tools/arb_eval_path.py [--parent-tree /path/to/built/parent/checkout] [--out profiles/arb_eval_path.txt]

Without --section this is a driver that never opens the GPU itself: it runs the sections one after the other as fresh processes,
each under its own `timeout`, and stops at the first one that fails.  Sections:
  A. device path per image: the ground truth's bytes uploaded from pageable memory, hat_pil_resize_u8, the encoder, the query at
     the ground truth's size into the workspace, hat_arb_psnr, two doubles back.
  B. host composition per image, what a user had to do before: Pillow's resize of the ground truth on the CPU, the LR image
     uploaded as fp32, `ESCLTE.upscale`, the fp32 image downloaded, the score in numpy.  With --parent-tree the package is
     imported from that (built) checkout of the parent commit; the numpy score is this file's own (the parent has none).
Both print the score, so the two paths can be compared; the network (default ESC-LTE, bf16, seeded random weights) is the same.
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 1020, 1356
SCALES = (2, 4, 12)
LIMITS = {"A": 300, "B": 300}      # seconds per section
med = statistics.median


def say(s=""):
    print(s, flush=True)


def _setup(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import super_resolution_amd.archs  # noqa: F401
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    torch.manual_seed(0)
    net = ESCLTE(compute_dtype="bf16").eval().to("cuda:0")
    gt = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np, torch, net, gt


def _sizes(s):
    h_lr, w_lr = H // s, W // s
    return (h_lr, w_lr), (h_lr * s, w_lr * s)


def section_a(args):
    np, torch, net, gt = _setup(ROOT)
    say(f"A. device path per image (ms), {H}x{W} ground truth, {torch.cuda.get_device_name(0)}, {args.warmup} warm-up + {args.frames} timed calls")
    for s in SCALES:
        (h_lr, w_lr), (h, w) = _sizes(s)
        call = lambda: net.score_gt_u8(torch.from_numpy(gt).to("cuda:0"), s, eval_type=f"div2k-{s}")
        for _ in range(args.warmup):
            score = call()
        ts = []
        for _ in range(args.frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score = call()                 # ends in the copy of the two sums: the device is idle when it returns
            ts.append((time.perf_counter() - t0) * 1e3)
        say(f"   x{s:<2d} LR {h_lr}x{w_lr}, grid {h}x{w}: median {med(ts):8.2f}  min {min(ts):.2f} max {max(ts):.2f}; PCIe {H * W * 3 / 1e6:.2f} MB up, "
            f"16 B down; div2k-{s} {score:.6f} dB")
    return 0


def host_score(np, pred, gt, shave):
    """esc_arb/utils.py calc_psnr, 'div2k': the clamped fp32 difference to byte / 255, shaved, squares summed in fp64."""
    d = np.clip(pred, np.float32(0), np.float32(1)) - (gt.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
    d = d[:, shave:-shave, shave:-shave].astype(np.float64)
    return -10.0 * np.log10((d * d).mean())


def section_b(args):
    tree = os.path.abspath(args.parent_tree) if args.parent_tree else ROOT
    np, torch, net, gt = _setup(tree)
    from PIL import Image
    import super_resolution_amd
    say(f"B. host composition per image (ms), package from {'the parent checkout' if args.parent_tree else 'this build'} "
        f"({os.path.relpath(os.path.dirname(super_resolution_amd.__file__), ROOT)}), Pillow {Image.__version__ if hasattr(Image, '__version__') else ''} on the CPU")
    for s in SCALES:
        (h_lr, w_lr), (h, w) = _sizes(s)
        parts = {"resize": [], "upload+upscale+download": [], "score": []}

        def call():
            t0 = time.perf_counter()
            lr = np.asarray(Image.fromarray(gt[:h, :w], "RGB").resize((w_lr, h_lr), Image.BICUBIC))
            t1 = time.perf_counter()
            x = (torch.from_numpy(lr).to(torch.float32) / 255).permute(2, 0, 1)[None].contiguous()
            y = net.upscale(x.to("cuda:0"), size=(h, w), scale_max=4)[0].cpu().numpy()
            t2 = time.perf_counter()
            score = host_score(np, y, gt[:h, :w], s + 6)
            t3 = time.perf_counter()
            return score, (t1 - t0, t2 - t1, t3 - t2)
        for _ in range(args.warmup):
            score, _ = call()
        ts = []
        for _ in range(args.frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score, p = call()
            ts.append((time.perf_counter() - t0) * 1e3)
            for k, v in zip(parts, p):
                parts[k].append(v * 1e3)
        say(f"   x{s:<2d} LR {h_lr}x{w_lr}, grid {h}x{w}: median {med(ts):8.2f}  min {min(ts):.2f} max {max(ts):.2f} ("
            + ", ".join(f"{k} {med(v):.2f}" for k, v in parts.items()) + f"); PCIe {h_lr * w_lr * 12 / 1e6:.2f} MB up, {h * w * 12 / 1e6:.2f} MB down; "
            f"div2k-{s} {score:.6f} dB")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["A", "B"], default=None, help="run one section in this process (the driver does that)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.section:
        return {"A": section_a, "B": section_b}[args.section](args)
    lines = []
    for sec in ("A", "B"):
        cmd = ["timeout", "-k", "10", str(LIMITS[sec]), sys.executable, os.path.abspath(__file__), "--section", sec, "--warmup", str(args.warmup),
               "--frames", str(args.frames)] + (["--parent-tree", args.parent_tree] if args.parent_tree and sec == "B" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines.extend(r.stdout.splitlines())
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:
            say(f"section {sec} ended with {r.returncode}: {r.stderr[-600:]}")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
