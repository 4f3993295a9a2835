"""tools/siting_path.py — what a co-sited chroma siting costs on the headline config (HAT-S x4, 720x1280 in, bf16, nv12).

    timeout -k 10 600 python tools/siting_path.py --out profiles/r16_siting_path.txt

One process; steps are chained and the first failure ends the run.  Reported (medians of rounds, every round's figure beside them):
  a. the two sited kernels against their centre instances, alone: to-planes at 720 x 1280 (padded to the window multiple) and
     from-planes at 2880 x 5120, HIP events around `steps` launches, the sitings alternated round by round.
  b. whole forward_yuv frames, nv12 in and out: siting 'center' (conv_last's fused epilogue) against 'left' and 'topleft'
     (hat_conv3x3_to_planes + the sited from-planes kernel), and 'left' in with a centre output (still fused), alternated round by
     round; beside them the byte estimate of the unfused ending: one fp32 output image written and read.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_path import H, S, W, build_net, device_ms  # noqa: E402


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

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def rounds_of(calls):
        ms = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        for _ in range(args.rounds):
            for k, fn in calls.items():
                ms[k].append(device_ms(fn, args.steps))
        return ms

    dev = torch.device("cuda:0")
    say(f"HAT-S x4 bf16, nv12 {H}x{W} -> {S * H}x{S * W}, {torch.cuda.get_device_name(0)}; {args.rounds} rounds x {args.steps} steps after "
        f"{args.warmup} warm-up calls, medians of rounds")
    rng = np.random.default_rng(0)
    f = torch.from_numpy(rng.integers(0, 256, (1,) + yuv.frame_shape(H, W), dtype=np.uint8)).to(dev)
    to_rgb, from_rgb = yuv.csc()
    # ---- a: the kernels alone
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    x = torch.empty(1, 3, Hp, Wp, device=dev)
    big = torch.rand(1, 3, S * H, S * W, device=dev)
    out = torch.empty((1,) + yuv.frame_shape(S * H, S * W), dtype=torch.uint8, device=dev)
    vin, vout = ops.yuv_views(f, "nv12"), ops.yuv_views(out, "nv12")
    calls = {}
    for s in yuv.SITINGS:
        calls[f"to-planes {s}"] = (lambda s=s: ops.yuv_to_planes(*vin, x, to_rgb, sub=(1, 1), siting=s))
        calls[f"from-planes {s}"] = (lambda s=s: ops.planes_to_yuv(big, *vout, from_rgb, sub=(1, 1), siting=s))
    ms = rounds_of(calls)
    in_mb = (f.numel() + x.numel() * 4) / 1e6
    out_mb = (big.numel() * 4 + out.numel()) / 1e6
    say(f"a. the kernels alone, us per launch; to-planes moves {in_mb:.1f} MB ({H}x{W} -> {Hp}x{Wp} fp32), from-planes {out_mb:.1f} MB")
    for k, v in ms.items():
        base = med(ms[k.split()[0] + " center"])
        mb = in_mb if k.startswith("to") else out_mb
        say(f"   {k:22s} median {med(v) * 1e3:8.1f} us ({(med(v) - base) * 1e3:+7.1f})  {mb / med(v) / 1e3:6.2f} TB/s   rounds "
            f"{' '.join(f'{t * 1e3:.1f}' for t in v)}")
    flush()
    # ---- b: whole frames
    net = build_net(dev)
    eng = net.engine()
    calls = {"center -> center (fused)": lambda: net.forward_yuv(f, fmt="nv12", out=out),
             "left -> center (fused)": lambda: net.forward_yuv(f, fmt="nv12", out=out, siting="left", out_siting="center"),
             "left -> left": lambda: net.forward_yuv(f, fmt="nv12", out=out, siting="left"),
             "topleft -> topleft": lambda: net.forward_yuv(f, fmt="nv12", out=out, siting="topleft")}
    counts = {}
    for k, fn in calls.items():
        before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
        fn()
        counts[k] = (eng.yuv_fused_calls - before[0], eng.yuv_planes_calls - before[1])
    ms = rounds_of(calls)
    base = med(ms["center -> center (fused)"])
    image_mb = 3 * S * H * S * W * 4 / 1e6
    say(f"b. forward_yuv nv12 -> nv12, ms per frame; the unfused ending writes and reads one fp32 image of {image_mb:.0f} MB "
        f"(byte estimate: 2 x {image_mb:.0f} MB, about 0.1 ms at the rate of a)")
    for k, v in ms.items():
        say(f"   {k:26s} median {med(v):.3f} ms ({med(v) - base:+.3f})  rounds {' '.join(f'{t:.3f}' for t in v)}   fused / planes endings "
            f"per call {counts[k][0]} / {counts[k][1]}")
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
