"""tools/escrealm_path.py — what an ESCRealM x2 forward costs at 1280x720 -> 2560x1440: the ESC_Real_X4-sized body
(n_blocks 10, conv_blocks 5, exp_ratio 2), bf16, with the unshuffled stem (the body runs at 640x360) and with `unshuffle_mod=False`
(the body at the full 1280x720: the only route to a x2 result without the stem), each with the "nearest+conv" and the "dysample"
head.  Report only, no gate; nothing here is tuned.

    timeout -k 10 900 python tools/escrealm_path.py [--out profiles/escrealm_path.txt]

One process.  After warm-up forwards, `--steps` forwards per configuration run under ops.profile() (HIP events around every
launch); reported are the wall time of a forward, and per kind of launch the count per forward, the median time of one launch and
the kind's share of the summed launch time; the new stem kernels' share is repeated on a line of its own."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BODY = dict(dim=64, pdim=16, kernel_size=13, n_blocks=10, conv_blocks=5, window_size=32, num_heads=4, upscaling_factor=2, exp_ratio=2)
STEM_KERNELS = ("unshuffle_pad_kernel", "escrealm_skip_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top", type=int, default=12)
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
    med = statistics.median
    h, w = 720, 1280
    say(f"ESCRealM x2 (10 blocks x 5 conv blocks, exp_ratio 2), bf16, {h}x{w} -> {2 * h}x{2 * w}, {torch.cuda.get_device_name(0)}; "
        f"{args.warmup} warm-up + {args.steps} timed + {args.steps} profiled forwards per configuration, medians")
    x = torch.rand(1, 3, h, w, device=dev)
    for up in ("nearest+conv", "dysample"):
        for unshuffle in (True, False):
            net = build_network(dict(BODY, type="ESCRealM", upsampler=up, mid_dim=48, unshuffle_mod=unshuffle, compute_dtype="bf16")).eval()
            net.load_state_dict(synth.synth_state_dict(net.state_dict(), 1234), strict=True)
            net = net.to(dev)
            with torch.no_grad():
                for _ in range(args.warmup):
                    y = net(x)
                torch.cuda.synchronize()
                wall = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    net(x)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                total, per = [], {}
                for _ in range(args.steps):
                    with ops.profile() as rec:
                        net(x)
                    torch.cuda.synchronize()
                    t = [(f"{name}  [{tag}]" if tag else name, s_.elapsed_time(e_)) for name, _, s_, e_, tag, _ in rec]
                    total.append(sum(q[1] for q in t))
                    for tag, ms in t:
                        per.setdefault(tag, []).append(ms)
            say()
            say(f"{up}, {'unshuffled stem (body 360x640)' if unshuffle else 'unshuffle_mod=False (body 720x1280)'}: out {tuple(y.shape)}, "
                f"{med(wall):.2f} ms per frame (eager, wall); {len(t)} launches, summed launch time median {med(total):.2f} ms")
            stem = sum(med(v) * (len(v) // args.steps) for k, v in per.items() if k.startswith(STEM_KERNELS))
            say(f"   new stem kernels (hat_unshuffle_pad, hat_escrealm_skip): {stem * 1e3:.1f} us, {100 * stem / med(total):.2f} % of the launch time")
            for tag, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:args.top]:
                ms, n = med(v), len(v) // args.steps
                say(f"   {tag:78s} x{n:<3d} median {ms * 1e3:9.1f} us  {100 * ms * n / med(total):5.1f} %")
            del net, y
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
