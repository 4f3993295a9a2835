"""tools/yuv_path.py — what the 4:2:0 frame path costs and saves on the headline config (HAT-S x4, 720x1280 in, bf16).

    timeout -k 10 900 python tools/yuv_path.py [--parent-tree /path/to/built/parent/checkout] [--out profiles/yuv_path.txt]

One process drives everything; steps are chained and the first failure ends the run.  Reported:
  A. conv_last with the planes, u8 and yuv420 epilogues (HIP events around each launch, one process);
     forward_u8 against forward_yuv420 per step, alternated round by round;
     the two standalone kernels (hat_yuv420_to_planes 720p, hat_planes_to_yuv420 2880x5120).
  B. host-to-host time per frame, numpy 4:2:0 in -> numpy 4:2:0 out: forward_u8 plus yuv.py's numpy colour conversion and
     subsampling on both sides (the status quo for a video user), forward_yuv420 with pageable copies, and
     frames.upscale_frames(pixfmt='i420') over --frames frames.
  C. with --parent-tree: `bench.py --gpus 1 --steps 20 --warmup 5` of the parent commit (a built checkout of it) and of this
     build as fresh processes, alternated; the spread between identical parent runs is printed beside the difference.
The CPU count in use is printed with B: it is a host-side number.
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
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from super_resolution_amd import frames as FR, ops, yuv
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
    seq = [rng.integers(0, 256, yuv.frame_shape(h, w), dtype=np.uint8) for _ in range(args.frames)]
    # ---- A: device time
    x = torch.rand(1, 3, h, w, device=dev)
    rgb8 = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, device=dev)
    out8 = torch.empty(1, s * h, s * w, 3, dtype=torch.uint8, device=dev)
    f420 = torch.from_numpy(seq[0]).to(dev).unsqueeze(0)
    out420 = torch.empty((1,) + yuv.frame_shape(s * h, s * w), dtype=torch.uint8, device=dev)
    for _ in range(args.warmup):
        net(x)
        net.forward_u8(rgb8, out=out8)
        net.forward_yuv420(f420, fmt="nv12", out=out420)
    say("A. device time")
    with ops.profile() as rec:
        for _ in range(3):
            net(x)
            net.forward_u8(rgb8, out=out8)
            net.forward_yuv420(f420, fmt="nv12", out=out420)
            net.forward_yuv420(f420, fmt="i420", out=out420)
    torch.cuda.synchronize()
    per = {}
    for name, _, s_, e_, tag, _ in rec:
        if "cab_squeeze_kernel<2" in name or "to_planes_kernel" in name:
            per.setdefault((name, tag), []).append(s_.elapsed_time(e_) * 1e3)
    for (name, tag), v in per.items():
        say(f"   {name:34s} median {med(v):8.1f} us  ({' '.join(f'{t:.1f}' for t in v)})   {tag}")
    u_ms, y_ms, i_ms = [], [], []
    for _ in range(args.rounds):                 # alternate the sides inside one process
        u_ms.append(device_ms(lambda: net.forward_u8(rgb8, out=out8), args.steps))
        y_ms.append(device_ms(lambda: net.forward_yuv420(f420, fmt="nv12", out=out420), args.steps))
        i_ms.append(device_ms(lambda: net.forward_yuv420(f420, fmt="i420", out=out420), args.steps))
    say(f"   forward_u8            per step: median {med(u_ms):.3f} ms  rounds {' '.join(f'{v:.3f}' for v in u_ms)}")
    say(f"   forward_yuv420 nv12   per step: median {med(y_ms):.3f} ms  rounds {' '.join(f'{v:.3f}' for v in y_ms)}")
    say(f"   forward_yuv420 i420   per step: median {med(i_ms):.3f} ms  rounds {' '.join(f'{v:.3f}' for v in i_ms)}")
    say(f"   forward_yuv420 nv12 - forward_u8 = {med(y_ms) - med(u_ms):+.3f} ms   (fused epilogue taken: {eng.yuv_fused_calls > 0}, "
        f"general route taken: {eng.yuv_planes_calls > 0})")
    to_rgb, from_rgb = yuv.csc()
    planes = torch.rand(1, 3, s * h, s * w, device=dev)
    for fmt in ("nv12", "i420"):
        v = ops.yuv420_views(out420, fmt)
        ops.planes_to_yuv420(planes, *v, from_rgb)
        ms = [device_ms(lambda: ops.planes_to_yuv420(planes, *v, from_rgb), args.steps) for _ in range(args.rounds)]
        say(f"   hat_planes_to_yuv420 {s * h}x{s * w} planes -> {fmt}: median {med(ms) * 1e3:.1f} us "
            f"({(planes.numel() * 4 + out420.numel()) / med(ms) / 1e9:.2f} TB/s)")
    xin = torch.zeros(1, 3, h, w, device=dev)
    for fmt in ("nv12", "i420"):
        v = ops.yuv420_views(f420, fmt)
        ms = [device_ms(lambda: ops.yuv420_to_planes(*v, xin, to_rgb), args.steps) for _ in range(args.rounds)]
        say(f"   hat_yuv420_to_planes {fmt} {h}x{w} -> planes: median {med(ms) * 1e3:.1f} us")
    del planes
    flush()
    # ---- B: host to host
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    say(f"B. host to host per frame (ms), numpy i420 in -> numpy i420 out; CPUs visible to the process {cpus}, torch threads {torch.get_num_threads()}")
    say(f"   copies: RGB route up {3 * h * w / 1e6:.1f} MB, down {3 * s * h * s * w / 1e6:.1f} MB; 4:2:0 route up {1.5 * h * w / 1e6:.1f} MB, "
        f"down {1.5 * s * h * s * w / 1e6:.1f} MB")

    def rgb_route(a, parts=None):
        t0 = time.perf_counter()
        p = yuv.yuv420_to_planes(a, fmt="i420")                                   # (1,3,h,w) float32
        r8 = np.rint(p[0].transpose(1, 2, 0) * np.float32(255.0)).astype(np.uint8)
        t1 = time.perf_counter()
        o8 = net.forward_u8(torch.from_numpy(r8).to(dev))[0].cpu().numpy()
        t2 = time.perf_counter()
        o = yuv.planes_to_yuv420((o8.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)[None], fmt="i420")[0]
        t3 = time.perf_counter()
        if parts is not None:
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return o

    def yuv_route(a):
        return net.forward_yuv420(torch.from_numpy(a).to(dev), fmt="i420")[0].cpu().numpy()

    n_b = min(args.frames, 6)
    a0, b0 = rgb_route(seq[0]), yuv_route(seq[0])
    d = np.abs(a0.astype(int) - b0.astype(int))
    say(f"   the RGB route rounds to 8-bit RGB on the way in and out, the 4:2:0 route does not: bytes differing {float((d > 0).mean()):.4f}, "
        f"max difference {int(d.max())}")
    rr, yy, parts = [], [], []
    for i in range(n_b):                         # alternate the two routes frame by frame
        t0 = time.perf_counter(); rgb_route(seq[i], parts); t1 = time.perf_counter(); yuv_route(seq[i]); t2 = time.perf_counter()
        rr.append((t1 - t0) * 1e3)
        yy.append((t2 - t1) * 1e3)
    say(f"   forward_u8 + numpy conversion on both sides:  median {med(rr):.1f}  ({' '.join(f'{v:.0f}' for v in rr)})")
    say(f"      of which numpy 4:2:0 -> RGB24 in {med([p[0] for p in parts]):.1f}, forward_u8 with copies {med([p[1] for p in parts]):.1f}, "
        f"numpy RGB24 -> 4:2:0 out ({s * h * s * w / 1e6:.1f} MP) {med([p[2] for p in parts]):.1f}")
    say(f"   forward_yuv420 with uint8 copies (pageable):  median {med(yy):.1f}  ({' '.join(f'{v:.0f}' for v in yy)})")
    for rep in range(2):
        t0 = time.perf_counter()
        n = sum(1 for _ in FR.upscale_frames(net, seq, pixfmt="i420"))
        dt = (time.perf_counter() - t0) * 1e3
        say(f"   upscale_frames(pixfmt='i420') over {n} frames (run {rep + 1}): {dt / n:.1f} ms per frame ({dt:.0f} ms in all, pinned buffers allocated inside)")
    flush()
    # ---- C: bench.py, parent against this build
    if args.parent_tree:
        say("C. bench.py --gpus 1 --steps 20 --warmup 5, fresh processes alternated")
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
