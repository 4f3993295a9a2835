"""tools/esclte_frame_path.py — what ESC-LTE's fused frame sinks save (the model of train_esc-lte.yaml: 5 x 5 blocks, hidden_dim 256),
for 720p -> 1080p (x1.5) and 720p -> x2, in both compute dtypes.

    timeout -k 10 900 python tools/esclte_frame_path.py [--out profiles/esclte_frame_path.txt] [--parent-dump parent.pt]

After one gen_feat per case, HIP events, warm-up, medians over the rounds, of the query alone:
  * fused: hat_lte_query_u8, and hat_lte_query_yuv into i420 and nv12 at 8 and 10 bits (ESCLTEEngine.query_grid_u8 / query_grid_yuv);
  * two-step: hat_lte_query's grid planes (ESCLTEEngine.query_grid, a fresh fp32 image per call) then hat_planes_to_u8 /
    hat_planes_to_yuv — the route a caller had before, and the one the tests hold the fused route equal to, bit for bit;
  * the device bytes each route allocates per call (peak above the level before the call), and whether the two results are equal.
The whole calls (upscale_u8 against u8_to_planes -> upscale -> planes_to_u8) are timed once per case for scale.

The plane path's bits against the parent commit: `--dump-upscale FILE`, run in a build of the parent, writes upscale() of golden case
a (tests/golden/esclte_a.npz, 20x24 -> 30x41) in both dtypes; `--parent-dump FILE` in this tree compares its own with torch.equal.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = dict(type="ESCLTE", dim=64, pdim=16, kernel_size=13, n_blocks=5, conv_blocks=5, window_size=32, num_heads=4, exp_ratio=1.25)
SINKS = [("u8", None, 8), ("i420", "i420", 8), ("nv12", "nv12", 8), ("i420 10-bit", "i420", 10), ("nv12 10-bit (P010)", "nv12", 10)]


def device_ms(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alloc_bytes(fn, dev):
    """Peak device bytes above the level before the call; what fn returns stays alive until after the reading."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    del keep
    return peak - before


def golden_upscale(dev):
    """upscale() of golden case a at its grid, (1,3,30,41) fp32 on the host, per compute dtype."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import esclte_ref as R
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    cfg, sd, g, meta = R.load_case("a")
    out = {}
    for dtype in ("bf16", "fp32"):
        net = build_network(dict(type="ESCLTE", **cfg, compute_dtype=dtype)).eval()
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            out[dtype] = net.to(dev).upscale(torch.from_numpy(g["x"]).to(dev) * 0.5 + 0.5, size=tuple(meta["what"]["grid"])).cpu()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump-upscale", default=None, metavar="FILE", help="write upscale() of golden case a in both dtypes and stop")
    ap.add_argument("--parent-dump", default=None, metavar="FILE", help="what --dump-upscale wrote in a build of the parent commit")
    args = ap.parse_args()
    import torch
    from super_resolution_amd import ops, synth, yuv
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    dev = torch.device("cuda:0")
    if args.dump_upscale:
        torch.save(golden_upscale(dev), args.dump_upscale)
        print(f"wrote {args.dump_upscale}")
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    med = statistics.median
    H, W = args.size
    say(f"ESC-LTE (5 x 5 blocks, hidden_dim 256), {H}x{W} in, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up, medians of {args.rounds} rounds")
    say("the query alone, after one gen_feat: fused sink | grid planes + conversion (two launches, a fresh fp32 image)")
    frame = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
    for dtype in ("bf16", "fp32"):
        net = build_network(dict(NET, compute_dtype=dtype)).eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
        net = net.to(dev)
        eng = net.engine(dev)
        for scale in (1.5, 2.0):
            h, w = int(H * scale), int(W * scale)
            cells = net._cells(H, W, h, w, 4)
            say(f"[{dtype}] x{scale}: {H}x{W} -> {h}x{w} ({h * w} queries; the fp32 image is {12 * h * w / 1e6:.1f} MB)")
            with torch.no_grad():
                whole = [device_ms(lambda: net.upscale_u8(frame, size=(h, w))) for _ in range(args.warmup + args.rounds)][args.warmup:]
                x = torch.empty(1, 3, H, W, device=dev)

                def whole_two_step():
                    ops.u8_to_planes(frame, x)
                    out = torch.empty(1, h, w, 3, dtype=torch.uint8, device=dev)
                    ops.planes_to_u8(net.upscale(x, size=(h, w)), out)
                    return out

                whole2 = [device_ms(whole_two_step) for _ in range(args.warmup + args.rounds)][args.warmup:]
                say(f"   whole call: upscale_u8 median {med(whole):8.2f} ms | u8_to_planes, upscale, planes_to_u8 median {med(whole2):8.2f} ms")
                net.upscale_u8(frame, size=(h, w))   # the features every query below reads
                for name, fmt, depth in SINKS:
                    if fmt is None:
                        dst, dst2 = (torch.empty(1, h, w, 3, dtype=torch.uint8, device=dev) for _ in range(2))
                        fused = lambda: eng.query_grid_u8(dst, cells, False)
                        convert = lambda p: ops.planes_to_u8(p[None], dst2)
                    else:
                        dt = torch.uint8 if depth == 8 else torch.uint16
                        sub, msb = yuv.LAYOUTS[fmt][:2], bool(yuv.container(depth, fmt, None)[3])
                        from_rgb = yuv.csc("bt601", False, depth)[1]
                        dst, dst2 = (torch.zeros((1,) + yuv.frame_shape_fmt(h, w, fmt), dtype=torch.int16 if depth != 8 else dt, device=dev).view(dt)
                                     for _ in range(2))
                        v1, v2 = ops.yuv_views(dst, fmt), ops.yuv_views(dst2, fmt)
                        fused = lambda: eng.query_grid_yuv(v1, cells, from_rgb, sub, depth, msb)
                        convert = lambda p: ops.planes_to_yuv(p[None], *v2, from_rgb, sub=sub, depth=depth, msb=msb)

                    def two_step():
                        p = eng.query_grid(h, w, cells, out_affine=(0.5, 0.5))
                        convert(p)
                        return p

                    t1 = [device_ms(fused) for _ in range(args.warmup + args.rounds)][args.warmup:]
                    t2 = [device_ms(two_step) for _ in range(args.warmup + args.rounds)][args.warmup:]
                    b1, b2 = alloc_bytes(fused, dev), alloc_bytes(two_step, dev)
                    raw = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
                    same = torch.equal(raw(dst), raw(dst2))
                    say(f"   {name:<20} fused median {med(t1):8.2f} ms ({' '.join(f'{v:.2f}' for v in t1)}), {b1 / 1e6:6.1f} MB allocated | two-step "
                        f"median {med(t2):8.2f} ms ({' '.join(f'{v:.2f}' for v in t2)}), {b2 / 1e6:6.1f} MB allocated | saved {med(t2) - med(t1):6.2f} ms "
                        f"| results {'equal' if same else 'DIFFER'}")
                    del dst, dst2
        del net, eng
    if args.parent_dump:
        parent, here = torch.load(args.parent_dump, weights_only=True), golden_upscale(dev)
        say("the plane path against the parent commit: upscale() of golden case a (20x24 -> 30x41), torch.equal of this tree's result and the parent's")
        for dtype in ("bf16", "fp32"):
            say(f"   [{dtype}] {'equal, bit for bit' if torch.equal(parent[dtype], here[dtype]) else 'DIFFERENT'} "
                f"(max-abs difference {float((parent[dtype] - here[dtype]).abs().max()):.3e})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
