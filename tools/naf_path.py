"""tools/naf_path.py — what the NAF stem of HybridHATNAF costs in front of HATX: HATX embed_dim 144, depths 6 x 6,
window 16 behind a 64-channel / 4-block stem, 720x1280 in, bf16.

    timeout -k 10 900 python tools/naf_path.py [--out profiles/r17_naf_path.txt]

One process.  After a warm-up forward, `--steps` forwards run under ops.profile() (HIP events around every launch); reported are
the median time per launch of hat_naf_half in its forms (a: stored stream; b: stream formed from the previous half; proj: the
last projection alone) and of hat_naf_fold, the achieved GB/s against the bytes model of the issue (per pixel: 4c in, and for
form b 4c out + the T-typed gated map in, + the gated map out), the stem's share of the summed launch time of the whole forward,
and, as the outside yardstick, the same stem composed from torch ops on the device (bf16, channels_last)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HATX = dict(upscale=2, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01, overlap_ratio=0.5,
            img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")


def torch_stem(sd, x, blocks):
    """x + tail(body(head(x))) from torch ops, bf16 channels_last."""
    import torch
    import torch.nn.functional as F
    p = {k: v.to(torch.bfloat16) for k, v in sd.items() if k.startswith("naf.")}
    conv = lambda t, k, **kw: F.conv2d(t, p[k + ".weight"], p[k + ".bias"], **kw)
    h = conv(x, "naf.head", padding=1)
    for i in range(blocks):
        b = f"naf.body.{i}"
        a, g = conv(conv(h, b + ".pw1"), b + ".dw", padding=1, groups=p[b + ".dw.weight"].shape[0]).chunk(2, dim=1)
        g = a * g
        y = h + p[b + ".beta"] * conv(g * conv(g.mean(dim=(2, 3), keepdim=True), b + ".sca.1"), b + ".pw2")
        a, g = conv(conv(y, b + ".ffn1"), b + ".ffn_dw", padding=1, groups=p[b + ".ffn_dw.weight"].shape[0]).chunk(2, dim=1)
        h = y + p[b + ".gamma"] * conv(a * g, b + ".ffn2")
    return x + conv(h, "naf.tail", padding=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
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
    width, blocks = 64, 4
    net = build_network(dict(type="HybridHATNAF", naf_width=width, naf_blocks=blocks, hat_kwargs=HATX, compute_dtype="bf16")).eval()
    sd = synth.synth_state_dict(net.state_dict(), 1234)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    med = statistics.median
    h, w = args.size
    say(f"HybridHATNAF: {width}-channel / {blocks}-block stem + HATX C=144 6x6 window 16 x2, bf16, {h}x{w}, {torch.cuda.get_device_name(0)}; "
        f"{args.warmup} warm-up + {args.steps} profiled forwards, medians")
    x = torch.rand(1, 3, h, w, device=dev)
    with torch.no_grad():
        for _ in range(args.warmup):
            net(x)
        torch.cuda.synchronize()
        stem_ms, all_ms, per = [], [], {}
        n_stem = 1 + 3 * blocks + 1 + 2          # head, (half, fold, half) per block, projection, tail, add: the first launches
        for _ in range(args.steps):
            with ops.profile() as rec:
                net(x)
            torch.cuda.synchronize()
            t = [(tag or name, s_.elapsed_time(e_), nbytes) for name, _, s_, e_, tag, nbytes in rec]
            stem_ms.append(sum(q[1] for q in t[:n_stem]))
            all_ms.append(sum(q[1] for q in t))
            for tag, ms, nbytes in t[:n_stem]:
                per.setdefault(tag, []).append((ms, nbytes))
        say(f"launches per forward {len(t)}, of which the stem's {n_stem}")
        for tag, v in per.items():
            ms = med([q[0] for q in v])
            rate = f"{v[0][1] / ms / 1e6:8.1f} GB/s of the bytes model ({v[0][1] / 1e9:.3f} GB)" if v[0][1] else ""
            say(f"   {tag:44s} x{len(v) // args.steps:<2d} median {ms * 1e3:9.1f} us  {rate}")
        say(f"stem: median {med(stem_ms):.3f} ms of {med(all_ms):.3f} ms summed launch time = {100 * med(stem_ms) / med(all_ms):.2f} % of the forward")
        # the outside yardstick
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        sdd = {k: v.to(dev) for k, v in sd.items() if k.startswith("naf.")}
        for _ in range(args.warmup):
            y_t = torch_stem(sdd, xb, blocks)
        ts = []
        for _ in range(args.steps):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            y_t = torch_stem(sdd, xb, blocks)
            e_.record()
            torch.cuda.synchronize()
            ts.append(s_.elapsed_time(e_))
        x_naf = net.engine()._workspace(1, h, w)["x_naf"]
        say(f"the same stem from torch ops (bf16, channels_last): median {med(ts):.3f} ms;  max |torch - HIP| of x_naf "
            f"{float((y_t.float() - x_naf).abs().max()):.3e}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
