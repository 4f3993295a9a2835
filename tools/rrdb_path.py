"""tools/rrdb_path.py — what an RRDBNet frame costs: 3x720x1280, x4, bf16, 23 blocks (RealESRGAN_x4plus / ESRGAN).
Report only, no gate.

    timeout -k 10 900 python tools/rrdb_path.py [--out profiles/rrdb_path.txt]

One process.  After warm-up calls of every shape and path that is timed:
  * ms per frame of `forward`, `upscale_u8` and `upscale_yuv` (nv12): `--windows` windows of `--steps` calls each between two device
    events, the profiler off; the median window and the spread (min .. max) over the windows;
  * us per launch class from `--psteps` forwards under ops.profile() (HIP events around every launch), medians, in a run of its
    own behind the end-to-end windows.
Then each of the five dense layers against its yardstick, hat_conv on the same layer and the same dense rows (convs 1-4 in place with
HAT_ACT_LRELU02; conv 5 with 0.2 folded, r1, fp32 rows out and NO T copy, which favours the yardstick): the two alternate, `--rounds`
rounds of `--lsteps` back-to-back launches each between two events; median, spread, ratio, and the layer's share of its FLOP bound
(2 * 9 * cin * cout FLOP per pixel over the bf16 MFMA peak, from the shapes)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_BF16_PEAK = 2.5e15   # FLOP/s, dense bf16 MFMA (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--psteps", type=int, default=3)
    ap.add_argument("--lsteps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rrdb_ref as R
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

    say(f"RRDBNet x4, 23 blocks, bf16, 3x{h}x{w} -> 3x{4 * h}x{4 * w}, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per path, "
        f"{args.windows} windows of {args.steps} calls, median (min .. max)")
    x = torch.rand(1, 3, h, w, device=dev)
    frame = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    nv12 = torch.randint(16, 236, (1, 3 * h // 2, w), dtype=torch.uint8, device=dev)
    net = build_network(dict(R.SURFACE_CFGS["x4_23"], type="RRDBNet", compute_dtype="bf16")).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
    net = net.to(dev)
    out_u8 = torch.empty(1, 4 * h, 4 * w, 3, dtype=torch.uint8, device=dev)
    out_yuv = torch.empty(1, 6 * h, 4 * w, dtype=torch.uint8, device=dev)
    eng = net.engine(dev)
    paths = [("forward", lambda: eng.forward(x)), ("upscale_u8", lambda: net.upscale_u8(frame, out=out_u8)),
             ("upscale_yuv nv12", lambda: net.upscale_yuv(nv12, fmt="nv12", out=out_yuv))]
    with torch.no_grad():
        for name, fn in paths:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            v = [window(fn, args.steps) for _ in range(args.windows)]
            say(f"   {name:18s} {med(v):8.3f} ms per frame ({min(v):.3f} .. {max(v):.3f})  {1e3 / med(v):6.1f} frames/s")
        per, total = {}, []
        for _ in range(args.psteps):
            with ops.profile() as rec:
                eng.forward(x)
            torch.cuda.synchronize()
            t = [(" ".join(tag.split()[:2]) + (" @" + tag.split()[2] if not tag.startswith("rdb") else ""), s_.elapsed_time(e_)) for _, _, s_, e_, tag, _ in rec]
            total.append(sum(q[1] for q in t))
            for c, ms in t:
                per.setdefault(c, []).append(ms)
        say(f"   per launch class ({args.psteps} profiled forwards of {len(t)} launches, summed launch time median {med(total):.3f} ms):")
        for c, v in per.items():
            say(f"      {c:28s} x{len(v) // args.psteps:<3d} median {med(v) * 1e3:8.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})  sum {med(v) * len(v) / args.psteps:7.3f} ms")
    del net, eng
    torch.cuda.empty_cache()

    # ---- the five dense layers against hat_conv on the same layer and the same dense rows ----
    dt, LD = ops.HAT_BF16, 192
    d = (torch.randn(1, h * w, LD, device=dev) * 0.5).to(torch.bfloat16)
    dn = torch.empty_like(d)
    r1 = torch.randn(1, h * w, 64, device=dev)
    s1, s2 = torch.empty_like(r1), torch.empty_like(r1)
    geo = dict(B=1, H=h, W=w, dtype=dt, ldx=LD)
    say()
    say(f"dense layers at {h}x{w}, bf16, hat_rdb_conv alternating with hat_conv on the same rows, {args.rounds} rounds of {args.lsteps} launches, "
        f"median us (min .. max):")
    for cin in ops.RDB_CIN:
        cout = 64 if cin == 192 else 32
        wt, b = synth.normal(5, f"w{cin}", (cout, cin, 3, 3), std=(9 * cin) ** -0.5), synth.normal(5, f"b{cin}", (cout,), std=0.1)
        pr = ops.pack_rdb_conv(wt, b, dt, dev)
        if cin < 192:
            pw = ops.pack_conv_weight(wt, b, dt, dev)
            mine = lambda: ops.rdb_conv(pr, d, d, **geo, ldo=LD, out_off=cin, slope=0.2)
            ref = lambda: ops.conv(pw, d, d.view(-1)[cin:], **geo, ldo=LD, act=ops.ACT_LRELU02, n_store=32)
        else:
            pw = ops.pack_conv_weight(wt, b, dt, dev, scale=0.2)
            mine = lambda: ops.rdb_conv(pr, d, dn, **geo, ldo=LD, out_off=0, beta1=0.2, r1=r1, s_out=s1)
            ref = lambda: ops.conv(pw, d, s2, **geo, ldo=64, out_mode=ops.O_NHWC_F32, r1=r1, ldr1=64)
        for _ in range(args.warmup):
            mine(), ref()
        torch.cuda.synchronize()
        tv, tr = [], []
        for _ in range(args.rounds):
            tv.append(window(mine, args.lsteps))
            tr.append(window(ref, args.lsteps))
        mv, mr = med(tv), med(tr)
        flop = 2.0 * 9 * cin * cout * h * w
        say(f"   conv {cin:3d} -> {cout}: hat_rdb_conv {mv * 1e3:7.1f} ({min(tv) * 1e3:.1f} .. {max(tv) * 1e3:.1f})   hat_conv {mr * 1e3:7.1f} ({min(tr) * 1e3:.1f} .. {max(tr) * 1e3:.1f})   "
            f"ratio {mv / mr:.3f}; spread {(max(tv) - min(tv)) / mv * 100:.1f} % / {(max(tr) - min(tr)) / mr * 100:.1f} % of the medians; "
            f"{flop / 1e9:.1f} GFLOP -> {flop / MFMA_BF16_PEAK * 1e6:.1f} us at peak, hat_rdb_conv at {100 * flop / MFMA_BF16_PEAK / (mv * 1e-3):.1f} %, hat_conv at "
            f"{100 * flop / MFMA_BF16_PEAK / (mr * 1e-3):.1f} %")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
