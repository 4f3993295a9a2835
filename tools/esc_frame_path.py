"""tools/esc_frame_path.py — what the ESC family's frame paths save on a 1280x720 frame, for ESC x4 and for ESCReal (default head).

    timeout -k 10 600 python tools/esc_frame_path.py --parent-tree <built parent checkout> [--out profiles/esc_frame_path.txt]

Per network, in bf16, HIP events, warm-up, medians over the timed runs (>= 20):
  * this tree: `upscale_u8` and `upscale_yuv(fmt='nv12')` on a device frame, with out= (the steady state of frames.upscale_frames), and
    beside them, alternating with them run by run, the planes route on the same tree (hat_u8_to_planes / hat_yuv_to_planes,
    `forward`, hat_planes_to_u8 / hat_planes_to_yuv), which the tests hold the calls equal to, bit for bit;
  * the parent tree (a fresh process whose imports come from --parent-tree): what a user had to do there — upload the frame as fp32
    planes (pinned, 12 bytes a pixel), `forward`, ops.planes_to_u8 / ops.planes_to_yuv (another process: it cannot alternate
    with this tree's runs, so small differences against it say nothing);
  * the bytes of workspace the fused sinks no longer write (the fp32 image) and the bytes no longer uploaded.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = dict(dim=64, pdim=16, kernel_size=13, n_blocks=5, conv_blocks=5, window_size=32, num_heads=4, exp_ratio=1.25)
NETS = {"ESC x4": dict(BODY, type="ESC", upscaling_factor=4), "ESCReal (default head, x4)": dict(BODY, type="ESCReal", upscaling_factor=4)}


def device_ms(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def timed(fn, warmup, runs):
    return [device_ms(fn) for _ in range(warmup + runs)][warmup:]


def alternating(fns, warmup, runs):
    """The routes of one comparison timed in turn, run by run (a, b, a, b ...), so that clock and thermal drift fall on all alike."""
    t = [[] for _ in fns]
    for i in range(warmup + runs):
        for k, fn in enumerate(fns):
            ms = device_ms(fn)
            if i >= warmup:
                t[k].append(ms)
    return t


def build(name, dev):
    import torch
    import super_resolution_amd.archs  # noqa: F401
    from super_resolution_amd import synth
    from super_resolution_amd.registry import build_network
    net = build_network(dict(NETS[name], compute_dtype="bf16")).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
    return net.to(dev)


def planes_route(net, H, W, dev, warmup, runs, upload, calls=False):
    """The planes route of a tree, per sink -> {sink: [ms]}; calls: -> {sink: the callable}, untimed.  upload: the frame arrives as pinned fp32 planes on the host (the parent's
    user); else as a device byte / nv12 frame converted by hat_u8_to_planes / hat_yuv_to_planes."""
    import torch
    from super_resolution_amd import ops, yuv
    S = net.upscale
    x = torch.empty(1, 3, H, W, device=dev)
    host = torch.rand(1, 3, H, W).pin_memory()
    u8 = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
    nv12 = torch.randint(16, 236, (1, 3 * H // 2, W), dtype=torch.uint8, device=dev)
    to_rgb, from_rgb = yuv.csc("bt601", False, 8)
    out8 = torch.empty(1, S * H, S * W, 3, dtype=torch.uint8, device=dev)
    outy = torch.empty(1, 3 * S * H // 2, S * W, dtype=torch.uint8, device=dev)

    def run_u8():
        if upload:
            x.copy_(host, non_blocking=True)
        else:
            ops.u8_to_planes(u8, x)
        ops.planes_to_u8(net(x).float().contiguous(), out8)

    def run_nv12():
        if upload:
            x.copy_(host, non_blocking=True)
        else:
            ops.yuv_to_planes(*ops.yuv_views(nv12, "nv12"), x, to_rgb, sub=(1, 1))
        ops.planes_to_yuv(net(x).float().contiguous(), *ops.yuv_views(outy, "nv12"), from_rgb, sub=(1, 1))

    if calls:
        return {"u8": run_u8, "nv12": run_nv12}
    with torch.no_grad():
        return {"u8": timed(run_u8, warmup, runs), "nv12": timed(run_nv12, warmup, runs)}


def measure_parent(args):
    """Runs in the child process: imports resolve to the parent tree; one JSON line on stdout."""
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    dev = torch.device("cuda:0")
    H, W = args.size
    print("PARENT " + json.dumps({name: planes_route(build(name, dev), H, W, dev, args.warmup, args.runs, upload=True) for name in NETS}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, metavar="DIR", help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--measure-parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.measure_parent:
        return measure_parent(args)
    parent = None
    if args.parent_tree:   # first, and in a process of its own: the two trees' libraries never share a process
        tree = os.path.abspath(args.parent_tree)
        cmd = [sys.executable, os.path.abspath(__file__), "--measure-parent", "--tree", tree, "--runs", str(args.runs), "--warmup",
               str(args.warmup), "--size", *map(str, args.size)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=tree)
        if r.returncode != 0:
            raise RuntimeError(f"the parent tree's run failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        parent = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("PARENT "))[7:])
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda:0")
    H, W = args.size
    med, lines = statistics.median, []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"the ESC family's frame paths, {W}x{H} in, bf16, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up, medians of {args.runs} runs (HIP events)")
    for name in NETS:
        net = build(name, dev)
        eng, S = net.engine(dev), net.upscale
        u8 = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
        nv12 = torch.randint(16, 236, (1, 3 * H // 2, W), dtype=torch.uint8, device=dev)
        out8 = torch.empty(1, S * H, S * W, 3, dtype=torch.uint8, device=dev)
        outy = torch.empty(1, 3 * S * H // 2, S * W, dtype=torch.uint8, device=dev)
        planes = planes_route(net, H, W, dev, args.warmup, args.runs, upload=False, calls=True)
        with torch.no_grad():   # the call and the planes route of the same tree alternate run by run
            t8, p8 = alternating([lambda: net.upscale_u8(u8, out=out8), planes["u8"]], args.warmup, args.runs)
            ty, py = alternating([lambda: net.upscale_yuv(nv12, fmt="nv12", out=outy), planes["nv12"]], args.warmup, args.runs)
        here = {"u8": p8, "nv12": py}
        routes = f"u8 fused {eng.u8_fused_calls} planes {eng.u8_planes_calls}, yuv fused {eng.yuv_fused_calls} planes {eng.yuv_planes_calls}"
        say(f"[{name}] {W}x{H} -> {S * W}x{S * H}   (sink calls: {routes})")
        for sink, t in (("u8", t8), ("nv12", ty)):
            call = "upscale_u8" if sink == "u8" else "upscale_yuv(fmt='nv12')"
            line = (f"   {sink:<5} this tree {call:<24} median {med(t):8.2f} ms (min {min(t):.2f}, max {max(t):.2f}) | this tree, planes route "
                    f"(alternating) median {med(here[sink]):8.2f} ms (min {min(here[sink]):.2f}, max {max(here[sink]):.2f})")
            if parent is not None:
                p = parent[name][sink]
                line += f" | parent: upload fp32 planes, forward, planes_to_{'u8' if sink == 'u8' else 'yuv'} median {med(p):8.2f} ms (min {min(p):.2f}, max {max(p):.2f})"
            say(line)
        say(f"   the fp32 image a fused sink does not write: {12 * S * S * H * W / 1e6:.1f} MB of workspace; uploaded per frame: "
            f"{3 * H * W / 1e6:.1f} MB of bytes ({1.5 * H * W / 1e6:.1f} MB as nv12) in place of {12 * H * W / 1e6:.1f} MB of fp32 planes")
        del net, eng
    # the sinks alone: hat_shuffle_to_u8 / hat_shuffle_to_yuv against the two launches they replace, on x4 rows of this frame size
    from super_resolution_amd import ops, yuv
    s_, ld = 4, 48
    rows, base = torch.rand(1, H * W, ld, device=dev), torch.rand(1, 3, H, W, device=dev)
    y = torch.empty(1, 3, s_ * H, s_ * W, device=dev)
    o8 = torch.empty(1, s_ * H, s_ * W, 3, dtype=torch.uint8, device=dev)
    views = ops.yuv_views(torch.empty(1, 3 * s_ * H // 2, s_ * W, dtype=torch.uint8, device=dev), "nv12")
    m, geo = yuv.csc("bt601", False, 8)[1], dict(B=1, H=H, W=W, s=s_, ld=ld)
    say(f"the sinks alone, x{s_} rows (ld {ld}) of a {W}x{H} map, microseconds: fused | the two launches it replaces")
    for name, fused, two in (
            ("u8, base image", lambda: ops.shuffle_to_u8(rows, base, o8, **geo), lambda: (ops.esc_shuffle_add(rows, base, y, **geo), ops.planes_to_u8(y, o8))),
            ("nv12, base image", lambda: ops.shuffle_to_yuv(rows, base, *views, m, sub=(1, 1), **geo),
             lambda: (ops.esc_shuffle_add(rows, base, y, **geo), ops.planes_to_yuv(y, *views, m, sub=(1, 1)))),
            ("u8, no base", lambda: ops.shuffle_to_u8(rows, None, o8, **geo), lambda: (ops.shuffle_planes(rows, y, **geo), ops.planes_to_u8(y, o8)))):
        t1, t2 = alternating([fused, two], args.warmup, args.runs)
        say(f"   {name:<18} fused median {1e3 * med(t1):7.1f} (min {1e3 * min(t1):.1f}, max {1e3 * max(t1):.1f}) | two-step median {1e3 * med(t2):7.1f} "
            f"(min {1e3 * min(t2):.1f}, max {1e3 * max(t2):.1f})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
