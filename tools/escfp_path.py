"""tools/escfp_path.py — what the launches of an ESCFP forward cost: the full ESC_FP_X4 config (n_blocks 5,
conv_blocks 5, exp_ratio 1.25) on a 320x180 low-resolution frame, bf16.  Report only, no gate.

    timeout -k 10 600 python tools/escfp_path.py [--out profiles/r20_escfp_path.txt]

One process.  After warm-up forwards, `--steps` forwards run under ops.profile() (HIP events around every launch); reported are, per
kind of launch, the count per forward, the median time of one launch, the kind's share of the summed launch time, and where the
wrapper has a bytes model the achieved GB/s against it.  hat_escfp_convffn's model is the derived HBM traffic of a launch: 192 B/px
in (48 fp32 channels; the residual, where there is one, as much again) and 96 (T rows) or 192 (fp32 rows) B/px out."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESC_FP_X4 = dict(dim=48, pdim=16, kernel_size=13, n_blocks=5, conv_blocks=5, window_size=32, num_heads=3, upscaling_factor=4, exp_ratio=1.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from super_resolution_amd import ops, synth
    from super_resolution_amd.registry import build_network
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    med = statistics.median
    h, w = 180, 320
    say(f"ESC_FP_X4 (5 blocks x 5 conv blocks, exp_ratio 1.25), bf16, {h}x{w} -> {4 * h}x{4 * w}, {torch.cuda.get_device_name(0)}; "
        f"{args.warmup} warm-up + {args.steps} profiled forwards, medians")
    x = torch.rand(1, 3, h, w, device=dev)
    net = build_network(dict(ESC_FP_X4, type="ESCFP", compute_dtype="bf16")).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
    net = net.to(dev)
    with torch.no_grad():
        for _ in range(args.warmup):
            net(x)
        torch.cuda.synchronize()
        total, per = [], {}
        for _ in range(args.steps):
            with ops.profile() as rec:
                net(x)
            torch.cuda.synchronize()
            t = [(f"{name}  [{tag}]" if tag else name, s_.elapsed_time(e_), nbytes) for name, _, s_, e_, tag, nbytes in rec]
            total.append(sum(q[1] for q in t))
            for tag, ms, nbytes in t:
                per.setdefault(tag, []).append((ms, nbytes))
    say()
    say(f"{len(t)} launches per forward, summed launch time median {med(total):.3f} ms")
    for tag, v in sorted(per.items(), key=lambda kv: -sum(q[0] for q in kv[1])):
        ms, n = med([q[0] for q in v]), len(v) // args.steps
        rate = f"  {v[0][1] / ms / 1e6:7.1f} GB/s of {v[0][1] / 1e9:.3f} GB" if v[0][1] else ""
        say(f"   {tag:78s} x{n:<3d} median {ms * 1e3:9.1f} us  {100 * ms * n / med(total):5.1f} %{rate}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
