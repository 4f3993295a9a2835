"""tools/packed_path.py — what the packed 4:2:2 frame boundary costs on the headline config (HAT-S x4, 720x1280 in, bf16).

    timeout -k 10 600 python tools/packed_path.py --out profiles/packed422_path.txt

One process, one frame.  Reported (medians of rounds, HIP events around the calls, every round's figure beside them):
  a. hat_packed422_to_planes (720p frame -> padded fp32 planes) and hat_planes_to_packed422 (2880 x 5120 planes -> frame) per
     layout, centre- and left-sited, with the planar 'i422' kernels of the same tree beside them.
  b. a whole forward_yuv(uyvy -> uyvy) against forward_yuv(i422 -> i422), alternated round by round; the planar call's
     centre-sited output is written in conv_last's epilogue, the packed call's from fp32 planes.
Descriptive numbers for DESIGN.md §4.24: no bar is attached to them.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

from chroma_path import H, S, W, build_net, device_ms  # noqa: E402

LAYOUTS = (("uyvy", 8), ("yuy2", 8), ("y210", 10), ("v210", 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from super_resolution_amd import ops, yuv
    lines = []
    med = statistics.median

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = [device_ms(fn, args.steps) for _ in range(args.rounds)]
        return med(ms), " ".join(f"{v:.3f}" for v in ms)

    dev = torch.device("cuda:0")
    dt = lambda side: torch.int16 if side.dtype is torch.uint16 else torch.uint8
    say(f"HAT-S x4 bf16, {H}x{W} -> {S * H}x{S * W}, {torch.cuda.get_device_name(0)}; {args.rounds} rounds x {args.steps} steps after "
        f"{args.warmup} warm-up calls, medians of rounds (ms), every round beside them")
    say("a. the frame-boundary kernels alone, one frame")
    x = torch.empty(1, 3, H, W, device=dev)
    y = torch.rand(1, 3, S * H, S * W, device=dev)
    for siting in ("center", "left"):
        for fmt, depth in LAYOUTS + (("i422", 8), ("i422", 10)):
            side = ops.FrameSide(fmt, depth=depth, siting=siting)
            to_rgb, from_rgb = yuv.csc(depth=depth)
            rng = np.random.default_rng(0)
            src = torch.from_numpy(rng.integers(0, 256, (1,) + side.shape(H, W), dtype=np.uint8).astype(np.int16 if dt(side) is torch.int16 else np.uint8))
            src = src.to(dev).view(side.dtype)
            dst = torch.zeros((1,) + side.shape(S * H, S * W), dtype=dt(side), device=dev).view(side.dtype)
            m_in, r_in = timed(lambda: side.to_planes(src, x, to_rgb, width=W))
            m_out, r_out = timed(lambda: side.from_planes(y, dst, from_rgb, width=S * W))
            gb_in = (src.numel() * src.element_size() + x.numel() * 4) / 1e9
            gb_out = (dst.numel() * dst.element_size() + y.numel() * 4) / 1e9
            say(f"   {fmt:5s} {depth:2d}-bit {siting:6s}  to planes {m_in:7.3f} ms ({gb_in / m_in * 1e3:6.0f} GB/s)  [{r_in}]   "
                f"from planes {m_out:7.3f} ms ({gb_out / m_out * 1e3:6.0f} GB/s)  [{r_out}]")
    say("b. a whole frame call, alternated round by round")
    net = build_net(dev)
    calls = {}
    for fmt in ("i422", "uyvy"):
        side = ops.FrameSide(fmt)
        f = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1,) + side.shape(H, W), dtype=np.uint8)).to(dev)
        out = torch.empty((1,) + side.shape(S * H, S * W), dtype=torch.uint8, device=dev)
        calls[fmt] = (lambda f=f, out=out, fmt=fmt: net.forward_yuv(f, fmt=fmt, out=out))
        for _ in range(args.warmup):
            calls[fmt]()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn, args.steps))
    for k in calls:
        say(f"   forward_yuv {k} -> {k}   {med(ms[k]):8.3f} ms   [{' '.join(f'{v:.3f}' for v in ms[k])}]")
    say(f"   uyvy - i422: {med(ms['uyvy']) - med(ms['i422']):+.3f} ms; fused epilogues so far {net.engine().yuv_fused_calls}, from-planes endings "
        f"{net.engine().yuv_planes_calls}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
