"""tools/srvgg_path.py — what an SRVGGNetCompact frame costs: 3x720x1280, x4, bf16, num_conv 16 and 32 (the two published
configurations).  Report only, no gate.

    timeout -k 10 600 python tools/srvgg_path.py [--out profiles/srvgg_path.txt]

One process.  Per configuration, after warm-up calls of every shape and path that is timed:
  * ms per frame of `forward`, `upscale_u8` and `upscale_yuv` (nv12): `--windows` windows of `--steps` calls each between two device
    events, the profiler off; the median window and the spread (min .. max) over the windows;
  * us per launch class (first conv, body layer, last conv, head) from `--steps` forwards under ops.profile() (HIP events around every
    launch), medians, in a run of its own behind the end-to-end windows.
Then the body layer against its yardstick, the parent's resident-weight kernel on the same shape (hat_conv, 64 -> 64, 3x3, bf16, no
activation, which dispatches to conv64r_kernel): the two alternate, `--rounds` rounds of `--steps` back-to-back launches each between
two events; median, spread, ratio, and the body layer's share of its own bounds — 2 * 9 * 64 * 64 FLOP per pixel over the bf16 MFMA
peak, and 2 * 64 * 2 bytes per pixel over the HBM peak (each row read once and written once), both from the shapes."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_BF16_PEAK = 2.5e15   # FLOP/s, dense bf16 MFMA (spec)
HBM_PEAK = 8.0e12         # bytes/s (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import srvgg_ref as R
    from super_resolution_amd import ops, synth
    from super_resolution_amd.registry import build_network
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    med = statistics.median
    h, w = 720, 1280

    def window(fn, n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    def windows(fn, n, k):
        v = [window(fn, n) for _ in range(k)]
        return med(v), min(v), max(v)

    say(f"SRVGGNetCompact x4, prelu, bf16, 3x{h}x{w} -> 3x{4 * h}x{4 * w}, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per path, "
        f"{args.windows} windows of {args.steps} calls, median (min .. max)")
    x = torch.rand(1, 3, h, w, device=dev)
    frame = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    nv12 = torch.randint(16, 236, (1, 3 * h // 2, w), dtype=torch.uint8, device=dev)
    classes = {"vgg 3->64": "first conv", "vgg 64->64": "body layer", "k3 64->48": "last conv", "shuffle": "head"}
    for nconv in (16, 32):
        net = build_network(dict(R.SURFACE_CFGS[f"x4_{nconv}"], type="SRVGGNetCompact", compute_dtype="bf16")).eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
        net = net.to(dev)
        out_u8 = torch.empty(1, 4 * h, 4 * w, 3, dtype=torch.uint8, device=dev)
        out_yuv = torch.empty(1, 6 * h, 4 * w, dtype=torch.uint8, device=dev)
        eng = net.engine(dev)
        paths = [("forward", lambda: eng.forward(x)), ("upscale_u8", lambda: net.upscale_u8(frame, out=out_u8)),
                 ("upscale_yuv nv12", lambda: net.upscale_yuv(nv12, fmt="nv12", out=out_yuv))]
        say()
        say(f"num_conv {nconv}: {nconv + 3} launches per forward")
        with torch.no_grad():
            for name, fn in paths:
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                m, lo, hi = windows(fn, args.steps, args.windows)
                say(f"   {name:18s} {m:7.3f} ms per frame ({lo:.3f} .. {hi:.3f})  {1e3 / m:6.1f} frames/s")
            per, total = {}, []
            for _ in range(args.steps):
                with ops.profile() as rec:
                    eng.forward(x)
                torch.cuda.synchronize()
                t = [(next((c for k, c in classes.items() if tag.startswith(k)), tag), s_.elapsed_time(e_)) for _, _, s_, e_, tag, _ in rec]
                total.append(sum(q[1] for q in t))
                for c, ms in t:
                    per.setdefault(c, []).append(ms)
            say(f"   per launch class (profiled forwards, summed launch time median {med(total):.3f} ms):")
            for c, v in per.items():
                say(f"      {c:12s} x{len(v) // args.steps:<3d} median {med(v) * 1e3:8.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        del net, eng

    # ---- the body layer against the parent's resident-weight kernel on the same shape ----
    dt = ops.HAT_BF16
    wt, b = synth.normal(5, "w", (64, 64, 3, 3), std=1 / 24), synth.normal(5, "b", (64,), std=0.1)
    pv = ops.pack_vgg_conv(wt, b, synth.uniform(5, "s", (64,)) - 0.3, dt, dev)
    pw = ops.pack_conv_weight(wt, b, dt, dev)
    rows = torch.randn(1, h * w, 64, device=dev).to(torch.bfloat16)
    o1, o2 = torch.empty_like(rows), torch.empty_like(rows)
    vgg = lambda: ops.vgg_conv(pv, rows, o1, B=1, H=h, W=w, dtype=dt)
    ref = lambda: ops.conv(pw, rows, o2, B=1, H=h, W=w, dtype=dt, ldx=64, ldo=64)
    for _ in range(args.warmup):
        vgg(), ref()
    torch.cuda.synchronize()
    tv, tr = [], []
    for _ in range(args.rounds):
        tv.append(window(vgg, args.steps))
        tr.append(window(ref, args.steps))
    mv, mr = med(tv), med(tr)
    flop, nbytes = 2.0 * 9 * 64 * 64 * h * w, 2.0 * 64 * 2 * h * w
    say()
    say(f"body layer 64 -> 64 at {h}x{w}, bf16, alternating with its yardstick, {args.rounds} rounds of {args.steps} launches, median (min .. max):")
    say(f"   hat_vgg_conv (slope epilogue)            {mv * 1e3:8.1f} us ({min(tv) * 1e3:.1f} .. {max(tv) * 1e3:.1f})")
    say(f"   hat_conv -> conv64r_kernel, HAT_ACT_NONE {mr * 1e3:8.1f} us ({min(tr) * 1e3:.1f} .. {max(tr) * 1e3:.1f})")
    say(f"   ratio hat_vgg_conv / yardstick {mv / mr:.3f}; yardstick spread {(max(tr) - min(tr)) / mr * 100:.1f} % of its median")
    say(f"   bounds from the shapes: {flop / 1e9:.1f} GFLOP -> {flop / MFMA_BF16_PEAK * 1e6:.1f} us at {MFMA_BF16_PEAK / 1e15:.1f} PFLOP/s; "
        f"{nbytes / 1e6:.0f} MB -> {nbytes / HBM_PEAK * 1e6:.1f} us at {HBM_PEAK / 1e12:.0f} TB/s")
    say(f"   hat_vgg_conv achieves {flop / (mv * 1e-3) / 1e12:.0f} TFLOP/s = {100 * flop / MFMA_BF16_PEAK / (mv * 1e-3):.1f} % of its FLOP bound and "
        f"{nbytes / (mv * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / HBM_PEAK / (mv * 1e-3):.1f} % of its byte bound")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
