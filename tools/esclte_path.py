"""tools/esclte_path.py — where the time of ESC-LTE goes (the model of train_esc-lte.yaml: 5 x 5 blocks, hidden_dim 256), for
720p -> 1080p (x1.5) and 720p -> x2, in both compute dtypes.

    timeout -k 10 900 python tools/esclte_path.py [--out profiles/esclte_path.txt]

Per case and dtype, HIP events, warm-up, medians over the rounds:
  * the encoder (every launch of gen_feat up to `last`), the coef | freq conv, and hat_lte_query in grid mode, from ops.profile();
  * the query kernel's achieved TFLOP/s against its FLOP model (ops.lte_query's `_timed` figure);
  * the same query computed with torch ops on the device in the compute dtype (the reference's query_rgb, statement for statement, in
    batches of 30000 queries as the reference's batched_predict takes them), on the engine's own coef / freq maps: what the kernel
    replaces.  Its result is compared with the kernel's first.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = dict(type="ESCLTE", dim=64, pdim=16, kernel_size=13, n_blocks=5, conv_blocks=5, window_size=32, num_heads=4, exp_ratio=1.25)


def make_coord(shape, dev):
    import torch
    seqs = [-1 + 1 / n + (2 / n) * torch.arange(n, device=dev).float() for n in shape]
    return torch.stack(torch.meshgrid(*seqs, indexing="ij"), dim=-1).view(-1, 2)


def torch_query(sd, coef, freq, inp, coord, cell, tdt):
    """lte.py:34-105 with torch ops; the MLP and its input in `tdt`, everything else in fp32."""
    import torch
    import torch.nn.functional as F
    H, W = coef.shape[-2:]
    fc = make_coord((H, W), coef.device).view(H, W, 2).permute(2, 0, 1).unsqueeze(0)
    near = lambda t, c: F.grid_sample(t, c.flip(-1).unsqueeze(1), mode="nearest", align_corners=False)[:, :, 0, :].permute(0, 2, 1)
    preds, areas = [], []
    for vy in (-1, 1):
        for vx in (-1, 1):
            c_ = coord.clone()
            c_[:, :, 0] += vy / H + 1e-6
            c_[:, :, 1] += vx / W + 1e-6
            c_.clamp_(-1 + 1e-6, 1 - 1e-6)
            q_coef, q_freq, q_coord = near(coef, c_), near(freq, c_), near(fc, c_)
            rel = (coord - q_coord) * torch.tensor([H, W], device=coord.device, dtype=torch.float32)
            rc = cell * torch.tensor([H, W], device=coord.device, dtype=torch.float32)
            q_freq = torch.stack(torch.split(q_freq, 2, dim=-1), dim=-1)
            q_freq = torch.sum(q_freq * rel.unsqueeze(-1), dim=-2) + F.linear(rc, sd["phase.weight"])
            x = (q_coef * torch.cat((torch.cos(math.pi * q_freq), torch.sin(math.pi * q_freq)), dim=-1)).to(tdt)
            for i in (0, 2, 4):
                x = F.relu(F.linear(x, sd[f"imnet.layers.{i}.weight"].to(tdt), sd[f"imnet.layers.{i}.bias"].to(tdt)))
            preds.append(F.linear(x.float(), sd["imnet.layers.6.weight"], sd["imnet.layers.6.bias"]))
            areas.append(torch.abs(rel[:, :, 0] * rel[:, :, 1]) + 1e-9)
    tot = torch.stack(areas).sum(dim=0)
    ret = sum(p * (a / tot).unsqueeze(-1) for p, a in zip(preds, areas[::-1]))
    return ret + F.grid_sample(inp, coord.flip(-1).unsqueeze(1), mode="bilinear", padding_mode="border", align_corners=False)[:, :, 0, :].permute(0, 2, 1)


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--bsize", type=int, default=30000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from super_resolution_amd import ops, synth
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    med = statistics.median
    H, W = args.size
    say(f"ESC-LTE (5 x 5 blocks, hidden_dim 256), {H}x{W} in, {torch.cuda.get_device_name(0)}; {args.warmup} warm-up, medians of {args.rounds} rounds")
    img = torch.rand(1, 3, H, W, device=dev)
    for dtype in ("bf16", "fp32"):
        net = build_network(dict(NET, compute_dtype=dtype)).eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
        net = net.to(dev)
        sd = {k: v.detach() for k, v in net.state_dict().items()}
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        for scale in (1.5, 2.0):
            h, w = int(H * scale), int(W * scale)
            with torch.no_grad():
                for _ in range(args.warmup):
                    y = net.upscale(img, scale=scale)
                torch.cuda.synchronize()
                t = {"enc": [], "cf": [], "q": []}
                flops = 0.0
                for _ in range(args.rounds):
                    with ops.profile() as rec:
                        net.upscale(img, scale=scale)
                    torch.cuda.synchronize()
                    ms = [(name, fl, s_.elapsed_time(e_)) for name, fl, s_, e_, _, _ in rec]
                    assert ms[-1][0].startswith("lte_query_kernel") and ms[-2][0].startswith("conv_kernel")
                    t["enc"].append(sum(m[2] for m in ms[:-2]))
                    t["cf"].append(ms[-2][2])
                    t["q"].append(ms[-1][2])
                    flops = ms[-1][1]
                wall = [device_ms(lambda: net.upscale(img, scale=scale), 1) for _ in range(args.rounds)]
                # the torch composition on the engine's own maps
                eng = net.engine(dev)
                ws, _, _ = eng._feat_ws
                cf = ws["cf"][0].view(H, W, 512).permute(2, 0, 1)[None]
                coef, freq, inp = cf[:, :256].contiguous(), cf[:, 256:].contiguous(), ws["x"]
                coord = make_coord((h, w), dev)[None]
                cell = torch.tensor([2 / h, 2 / w], device=dev).expand(h * w, 2)[None] * max(scale / 4, 1)

                def torch_path():
                    return torch.cat([torch_query(sd, coef, freq, inp, coord[:, i:i + args.bsize], cell[:, i:i + args.bsize], tdt)
                                      for i in range(0, h * w, args.bsize)], 1)

                for _ in range(args.warmup):
                    yt = torch_path()
                torch.cuda.synchronize()
                got = (y[0].permute(1, 2, 0).reshape(-1, 3) - 0.5) / 0.5
                d = (got - yt[0]).abs()
                tq = [device_ms(torch_path, 1) for _ in range(args.rounds)]
                del yt, got
            say(f"[{dtype}] x{scale}: {H}x{W} -> {h}x{w} ({h * w} queries)")
            say(f"   encoder (launches up to `last`)      median {med(t['enc']):9.2f} ms  (sum of per-launch HIP-event times)")
            say(f"   coef | freq conv 64 -> 512           median {med(t['cf']):9.2f} ms")
            say(f"   hat_lte_query, grid mode             median {med(t['q']):9.2f} ms   {flops / med(t['q']) / 1e9:7.1f} TFLOP/s of {flops / 1e12:.2f} TFLOP"
                f"  ({' '.join(f'{q:.2f}' for q in t['q'])})")
            say(f"   upscale(), one call, unprofiled      median {med(wall):9.2f} ms")
            say(f"   the query with torch ops ({tdt})   median {med(tq):9.2f} ms   = {med(tq) / med(t['q']):.2f} x the kernel;  kernel vs torch: max-abs "
                f"{float(d.max()):.3e}, mean-abs {float(d.mean()):.3e}")
        del net
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
