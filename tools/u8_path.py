"""tools/u8_path.py — what the 8-bit frame path costs and saves on the headline config (HAT-S x4, 720x1280 in, bf16).

    timeout -k 10 900 python tools/u8_path.py [--parent-tree /path/to/built/parent/checkout] [--out profiles/u8_path.txt]

One process drives everything; steps are chained and the first failure ends the run.  Reported:
  A. device time (HIP events) of forward_to_u8 against forward of this build, the two alternated round by round inside one
     process; with --parent-tree also forward of the parent commit (a built checkout of it), as fresh child processes
     alternated with children of this build (the spread between identical parent runs is printed beside the difference).
  B. host-to-host time per frame, numpy uint8 in -> numpy uint8 out: the float route (float32 / 255 on the host, upload,
     net, .cpu(), tensor2img) against forward_u8 with uint8 copies, and against frames.upscale_frames over --frames frames.
The CPU count in use and the copy sizes are printed with B: it is a host-side number.
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
if "--root" in sys.argv:   # a child measuring another checkout imports the package from there
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

HATS = dict(type="HAT", upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01,
            overlap_ratio=0.5, img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2,
            upsampler="pixelshuffle", resi_connection="1conv", compute_dtype="bf16")


def build_net(dev):
    import torch  # noqa: F401
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


def child_forward(args):
    """--child: device ms per forward() of the checkout --root names (default: this one), one figure per round."""
    import torch
    dev = torch.device("cuda:0")
    net = build_net(dev)
    x = torch.rand(1, 3, 720, 1280, device=dev)
    for _ in range(args.warmup):
        net(x)
    print(json.dumps({"forward_ms": [device_ms(lambda: net(x), args.steps) for _ in range(args.rounds)]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (A/B of forward)")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_forward(args)
    import numpy as np
    import torch
    from super_resolution_amd import frames as FR
    from super_resolution_amd.metrics import tensor2img
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    net = build_net(dev)
    eng = net.engine()
    med = statistics.median
    say(f"HAT-S x4 bf16, 720x1280 -> 2880x5120, {torch.cuda.get_device_name(0)}; {args.rounds} rounds x {args.steps} steps, medians of rounds")
    # ---- A: device time
    x = torch.rand(1, 3, 720, 1280, device=dev)
    out8 = torch.empty(1, 2880, 5120, 3, dtype=torch.uint8, device=dev)
    for _ in range(args.warmup):
        net(x)
        net.forward_to_u8(x, out=out8)
    f_ms, u_ms = [], []
    for _ in range(args.rounds):                 # alternate the two sides inside one process
        f_ms.append(device_ms(lambda: net(x), args.steps))
        u_ms.append(device_ms(lambda: net.forward_to_u8(x, out=out8), args.steps))
    say("A. device time per step (ms)")
    say(f"   forward        this build: median {med(f_ms):.3f}  rounds {' '.join(f'{v:.3f}' for v in f_ms)}")
    say(f"   forward_to_u8  this build: median {med(u_ms):.3f}  rounds {' '.join(f'{v:.3f}' for v in u_ms)}")
    say(f"   forward_to_u8 - forward = {med(u_ms) - med(f_ms):+.3f} ms   (fused epilogue taken: {eng.u8_fused_calls > 0})")
    from super_resolution_amd import ops
    with ops.profile() as rec:
        net(x)
        net.forward_to_u8(x, out=out8)
    torch.cuda.synchronize()
    for name, _, s, e, tag, _ in rec:
        if "cab_squeeze_kernel<2" in name:
            say(f"   {name:32s} {s.elapsed_time(e) * 1e3:8.1f} us   {tag}")
    # the general output route on its own: fp32 planes -> bytes, packed rows (dword stores) and an odd width (odd pitch: every
    # second row falls back to byte stores)
    planes = torch.rand(1, 3, 2880, 5120, device=dev)
    for ho, wo in ((2880, 5120), (2879, 5119)):
        o = torch.empty(1, ho, wo, 3, dtype=torch.uint8, device=dev)
        ops.planes_to_u8(planes, o)
        ms = [device_ms(lambda: ops.planes_to_u8(planes, o), args.steps) for _ in range(args.rounds)]
        say(f"   hat_planes_to_u8 2880x5120 planes -> {ho}x{wo} bytes: median {med(ms) * 1e3:.1f} us ({(planes.numel() * 4 + o.numel()) / med(ms) / 1e9:.2f} TB/s)")
    xin = torch.zeros(1, 3, 720, 1280, device=dev)
    fr = torch.randint(0, 256, (1, 718, 1275, 3), dtype=torch.uint8, device=dev)
    ms = [device_ms(lambda: ops.u8_to_planes(fr, xin), args.steps) for _ in range(args.rounds)]
    say(f"   hat_u8_to_planes 718x1275 bytes -> 720x1280 planes: median {med(ms) * 1e3:.1f} us")
    del planes
    if args.parent_tree:
        runs = {"parent": [], "branch": []}
        for i in range(2):
            for side, tree in (("parent", args.parent_tree), ("branch", None)):
                r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps),
                                    "--rounds", str(args.rounds), "--warmup", str(args.warmup)] + (["--root", tree] if tree else []),
                                   capture_output=True, text=True)
                if r.returncode != 0:
                    say(f"   child ({side}) failed with {r.returncode}: {r.stderr[-400:]}")
                    return 1
                runs[side].append(med(json.loads(r.stdout.strip().splitlines()[-1])["forward_ms"]))
        say(f"   forward, fresh processes alternated: parent commit {' '.join(f'{v:.3f}' for v in runs['parent'])} | this build "
            f"{' '.join(f'{v:.3f}' for v in runs['branch'])}")
        say(f"   spread of identical parent runs {max(runs['parent']) - min(runs['parent']):.3f} ms; this build - parent = "
            f"{med(runs['branch']) - med(runs['parent']):+.3f} ms")
    # ---- B: host to host
    rng = np.random.default_rng(0)
    seq = [rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8) for _ in range(args.frames)]
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    say(f"B. host to host per frame (ms), numpy uint8 in -> numpy uint8 out; CPUs visible to the process {cpus}, {torch.get_num_threads()} in use (torch threads {torch.get_num_threads()})")
    say(f"   copies: float route up {3 * 720 * 1280 * 4 / 1e6:.1f} MB, down {3 * 2880 * 5120 * 4 / 1e6:.1f} MB; u8 route up {3 * 720 * 1280 / 1e6:.1f} MB, "
        f"down {3 * 2880 * 5120 / 1e6:.1f} MB")

    def float_route(a):
        t = torch.from_numpy(a.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).contiguous().unsqueeze(0)
        return tensor2img(net(t.to(dev)).cpu())

    def u8_route(a):
        return net.forward_u8(torch.from_numpy(a).to(dev))[0].cpu().numpy()

    n_b = min(args.frames, 6)
    a8, b8 = float_route(seq[0]), u8_route(seq[0])
    say(f"   results equal: {bool(np.array_equal(a8, b8))}")
    fl, u8 = [], []
    for i in range(n_b):                         # alternate the two routes frame by frame
        t0 = time.perf_counter(); float_route(seq[i]); t1 = time.perf_counter(); u8_route(seq[i]); t2 = time.perf_counter()
        fl.append((t1 - t0) * 1e3)
        u8.append((t2 - t1) * 1e3)
    say(f"   float route (host /255, upload, net, .cpu(), tensor2img): median {med(fl):.1f}  ({' '.join(f'{v:.0f}' for v in fl)})")
    say(f"   forward_u8 with uint8 copies (pageable):                  median {med(u8):.1f}  ({' '.join(f'{v:.0f}' for v in u8)})")
    for rep in range(2):
        t0 = time.perf_counter()
        n = sum(1 for _ in FR.upscale_frames(net, seq))
        dt = (time.perf_counter() - t0) * 1e3
        say(f"   upscale_frames over {n} frames (run {rep + 1}): {dt / n:.1f} ms per frame ({dt:.0f} ms in all, pinned buffers allocated inside)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
