"""tools/deep_yuv_path.py — what 10-bit samples cost on the 4:2:0 frame path of the headline config (HAT-S x4, 720x1280 in, bf16).

    timeout -k 10 900 python tools/deep_yuv_path.py [--parent-tree /path/to/built/parent/checkout] [--out profiles/r10_deep_yuv_path.txt]

One process drives everything; steps are chained and the first failure ends the run.  Reported:
  A. conv_last with the yuv420 (8-bit) and yuv420p16 (10-bit, MSB-aligned) epilogues under ops.profile() (HIP events around
     each launch);
  B. forward_yuv420 8 -> 8, 8 -> 10 and 10 -> 10 (nv12 / P010) per step, alternated round by round; the spread of the 8 -> 8
     rounds is printed beside the differences;
  C. the two standalone kernels, bytes against words: hat_yuv420[p16]_to_planes 720p, hat_planes_to_yuv420[p16] 2880x5120;
  D. with --parent-tree: `bench.py --gpus 1 --steps 20 --warmup 5` of the parent commit (a built checkout of it) and of this
     build as fresh processes, alternated; the spread between identical parent runs is printed beside the difference.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HATS = dict(type="HAT", upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01,
            overlap_ratio=0.5, img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2,
            upsampler="pixelshuffle", resi_connection="1conv", compute_dtype="bf16")


def build_net(dev):
    from super_resolution_amd import synth
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(HATS)).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
    return net.to(dev)


def device_ms(fn, steps):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (A/B of bench.py)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from super_resolution_amd import ops, yuv
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dev = torch.device("cuda:0")
    net = build_net(dev)
    eng = net.engine()
    med = statistics.median
    h, w, s = 720, 1280, 4
    say(f"HAT-S x4 bf16, {h}x{w} -> {s * h}x{s * w}, {torch.cuda.get_device_name(0)}; {args.rounds} rounds x {args.steps} steps, medians of rounds")
    rng = np.random.default_rng(0)
    f8 = torch.from_numpy(rng.integers(0, 256, (1,) + yuv.frame_shape(h, w), dtype=np.uint8)).to(dev)
    f10 = torch.from_numpy((rng.integers(0, 1024, (1,) + yuv.frame_shape(h, w), dtype=np.uint16) << 6).view(np.int16)).to(dev).view(torch.uint16)
    o8 = torch.empty((1,) + yuv.frame_shape(s * h, s * w), dtype=torch.uint8, device=dev)
    o10 = torch.empty((1,) + yuv.frame_shape(s * h, s * w), dtype=torch.int16, device=dev).view(torch.uint16)
    routes = {"8 -> 8": lambda: net.forward_yuv420(f8, fmt="nv12", out=o8),
              "8 -> 10": lambda: net.forward_yuv420(f8, fmt="nv12", out=o10, out_depth=10),
              "10 -> 10": lambda: net.forward_yuv420(f10, fmt="nv12", out=o10, depth=10)}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    say("A. conv_last epilogues, device time per launch")
    with ops.profile() as rec:
        for _ in range(5):
            for fn in routes.values():
                fn()
    torch.cuda.synchronize()
    per = {}
    for name, _, s_, e_, tag, _ in rec:
        if "cab_squeeze_kernel<2" in name or "to_planes_kernel" in name:
            per.setdefault((name, tag), []).append(s_.elapsed_time(e_) * 1e3)
    for (name, tag), v in per.items():
        say(f"   {name:34s} median {med(v):8.1f} us  min {min(v):.1f} max {max(v):.1f} (n {len(v)})   {tag}")
    say("B. forward_yuv420 nv12 / P010, device time per step, routes alternated inside every round")
    ms = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            ms[k].append(device_ms(fn, args.steps))
    for k, v in ms.items():
        say(f"   {k:9s} median {med(v):.3f} ms  rounds {' '.join(f'{t:.3f}' for t in v)}")
    spread = max(ms["8 -> 8"]) - min(ms["8 -> 8"])
    say(f"   spread of the 8 -> 8 rounds {spread:.3f} ms; 8 -> 10 minus 8 -> 8 {med(ms['8 -> 10']) - med(ms['8 -> 8']):+.3f} ms; "
        f"10 -> 10 minus 8 -> 8 {med(ms['10 -> 10']) - med(ms['8 -> 8']):+.3f} ms  (fused epilogue taken: {eng.yuv_fused_calls > 0}, "
        f"general route taken: {eng.yuv_planes_calls > 0})")
    flush()
    say("C. standalone kernels")
    to_rgb, from_rgb = yuv.csc()
    planes = torch.rand(1, 3, s * h, s * w, device=dev)
    xin = torch.zeros(1, 3, h, w, device=dev)
    for fmt in ("nv12", "i420"):
        for out, kw, label in ((o8, {}, "bytes"), (o10, dict(depth=10, msb=fmt != "i420"), "10-bit words")):
            v = ops.yuv420_views(out, fmt)
            ops.planes_to_yuv420(planes, *v, from_rgb, **kw)
            t = [device_ms(lambda: ops.planes_to_yuv420(planes, *v, from_rgb, **kw), args.steps) for _ in range(args.rounds)]
            say(f"   planes {s * h}x{s * w} -> {fmt} {label}: median {med(t) * 1e3:.1f} us "
                f"({(planes.numel() * 4 + out.numel() * out.element_size()) / med(t) / 1e9:.2f} TB/s)")
        for src, kw, label in ((f8, {}, "bytes"), (f10, dict(depth=10, msb=fmt != "i420"), "10-bit words")):
            v = ops.yuv420_views(src, fmt)
            ops.yuv420_to_planes(*v, xin, to_rgb, **kw)
            t = [device_ms(lambda: ops.yuv420_to_planes(*v, xin, to_rgb, **kw), args.steps) for _ in range(args.rounds)]
            say(f"   {fmt} {label} {h}x{w} -> planes: median {med(t) * 1e3:.1f} us")
    del planes
    flush()
    # ---- D: bench.py, parent against this build
    if args.parent_tree:
        say("D. bench.py --gpus 1 --steps 20 --warmup 5, fresh processes alternated")
        runs = {"parent": [], "branch": []}
        del net, eng
        torch.cuda.empty_cache()
        for i in range(3):
            for side, tree in (("parent", os.path.abspath(args.parent_tree)), ("branch", ROOT)):
                r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20",
                                    "--warmup", "5"], capture_output=True, text=True, cwd=tree)
                if r.returncode != 0:
                    say(f"   bench.py ({side}) failed with {r.returncode}: {r.stderr[-400:]}")
                    flush()
                    return 1
                res = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
                runs[side].append(res)
        key = next((k for k in ("ms_per_step", "step_ms", "latency_ms", "ms") if k in runs["parent"][0]), None)
        say(f"   result keys: {sorted(runs['parent'][0])}")
        for side in ("parent", "branch"):
            say(f"   {side}: " + " | ".join(json.dumps({k: v for k, v in r.items() if isinstance(v, (int, float))}) for r in runs[side]))
        if key:
            pv, bv = [r[key] for r in runs["parent"]], [r[key] for r in runs["branch"]]
            say(f"   {key}: parent {' '.join(f'{v:.3f}' for v in pv)} | this build {' '.join(f'{v:.3f}' for v in bv)}")
            say(f"   spread of identical parent runs {max(pv) - min(pv):.3f}; this build - parent (medians) = {med(bv) - med(pv):+.3f}")
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
