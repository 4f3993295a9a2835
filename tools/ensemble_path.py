"""tools/ensemble_path.py — what the geometric self-ensemble costs beyond its eight forwards on the headline config (HAT-S x4,
720x1280 in, bf16).

    timeout -k 10 900 python tools/ensemble_path.py [--out profiles/r12_ensemble_path.txt]

One process; the three sides are alternated round by round and the medians of the rounds are reported:
  (a) forward_ensemble(x, 8): hat_dihedral_f32 makes the seven transformed inputs and undoes, scales and adds the eight outputs;
  (b) the eight member forwards alone, four at 720x1280 and four at 1280x720, on inputs transformed beforehand;
  (c) the same ensemble composed from torch ops on the device (flip / transpose / contiguous / mul / add around net(x)): what
      the kernel replaces.
(a) - (b) is the overhead of the kernel path, (c) - (b) that of the torch composition.  The two hat_dihedral_f32 kernels are
also timed per launch (HIP events) at the output size.  The results of (a) and (c) are compared bit for bit first.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

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


def member(x, i):
    import torch
    x = torch.flip(x, dims=[-1]) if i & 1 else x
    x = torch.flip(x, dims=[-2]) if i & 2 else x
    return (torch.transpose(x, -2, -1) if i & 4 else x).contiguous()


def undo(y, i):
    import torch
    y = torch.transpose(y, -2, -1) if i & 4 else y
    y = torch.flip(y, dims=[-2]) if i & 2 else y
    return torch.flip(y, dims=[-1]) if i & 1 else y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from super_resolution_amd import ops
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    net = build_net(dev)
    med = statistics.median
    (h, w), s, n = args.size, 4, 8
    say(f"HAT-S x4 bf16, {h}x{w} -> {s * h}x{s * w}, self-ensemble of {n}, {torch.cuda.get_device_name(0)}; {args.rounds} rounds x "
        f"{args.steps} steps, medians of rounds")
    x = torch.rand(1, 3, h, w, device=dev)
    xs = [member(x, i) for i in range(n)]

    def kernel_path():
        return net.forward_ensemble(x, n)

    def forwards_alone():
        for xi in xs:
            net(xi)

    def torch_path():
        acc = torch.zeros(1, 3, s * h, s * w, device=dev)
        for i in range(n):
            acc = acc + (1.0 / n) * undo(net(member(x, i)), i)
        return acc

    with torch.no_grad():
        for _ in range(args.warmup):
            a, _, c = kernel_path(), forwards_alone(), torch_path()
        torch.cuda.synchronize()
        say(f"forward_ensemble == torch composition, bit for bit: {bool(torch.equal(a, c))}")
        del a, c
        t = {"a": [], "b": [], "c": []}
        for _ in range(args.rounds):
            t["a"].append(device_ms(kernel_path, args.steps))
            t["b"].append(device_ms(forwards_alone, args.steps))
            t["c"].append(device_ms(torch_path, args.steps))
        fmt = lambda v: f"median {med(v):9.2f} ms  ({' '.join(f'{q:.2f}' for q in v)})"
        say(f"(a) forward_ensemble(x, 8)                      {fmt(t['a'])}")
        say(f"(b) the eight member forwards alone              {fmt(t['b'])}")
        say(f"(c) the ensemble composed from torch ops         {fmt(t['c'])}")
        oa, oc = med(t["a"]) - med(t["b"]), med(t["c"]) - med(t["b"])
        say(f"overhead of the kernel path (a) - (b): {oa:.2f} ms = {100 * oa / med(t['b']):.2f} % of the forwards;  of the torch composition "
            f"(c) - (b): {oc:.2f} ms = {100 * oc / med(t['b']):.2f} %")
        # the kernels alone, at the output size: 3 x sH x sW fp32 planes
        y = torch.rand(3, s * h, s * w, device=dev)
        yt = torch.rand(3, s * w, s * h, device=dev)
        acc = torch.zeros(3, s * h, s * w, device=dev)
        with ops.profile() as rec:
            for _ in range(5):
                for op in range(n):
                    ops.dihedral(yt if op & 4 else y, acc, op=op, inverse=True, alpha=1.0 / n, accumulate=op > 0)
        torch.cuda.synchronize()
        per = {}
        for name, _, s_, e_, tag, nbytes in rec:
            per.setdefault(tag, []).append((s_.elapsed_time(e_) * 1e3, nbytes))
        for tag, v in per.items():
            us = med([q[0] for q in v])
            say(f"   {tag:40s} median {us:8.1f} us   {v[0][1] / us / 1e6:6.2f} TB/s of algorithmic traffic")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
