"""tools/niqe_path.py — what NIQE costs on the device and on the host for one 2880x5120 frame (crop_border 4).

    timeout -k 10 600 python tools/niqe_path.py --pris-params niqe_pris_params.npz [--reps 5] [--out profiles/niqe_path.txt]

One process, steps in order, the first failure ends the run.  Reported:
  A. device time of the five NIQE launches (Y, the two half-size passes, the two block kernels) under ops.profile();
  B. niqe.calculate_niqe on the host for the same frame, in this process (CPU count printed);
  C. the score difference.
The pristine model is data of the reference: --pris-params, or $HAT_NIQE_PRIS_PARAMS (niqe.pris_params).
"""
from __future__ import annotations

import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame(rng, h, w):
    """a blocky smooth image plus noise of sigma 4 (the shape of an SR result)"""
    import numpy as np
    low = rng.integers(30, 226, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    a = np.repeat(np.repeat(low, 8, axis=0), 8, axis=1)[:h, :w]
    return np.clip(np.round(a + rng.normal(0.0, 4.0, a.shape).astype(np.float32)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pris-params", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from super_resolution_amd import niqe, ops
    from super_resolution_amd.metrics_device import calculate_niqe_u8
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    pris = niqe.pris_params(args.pris_params)
    dev = torch.device("cuda:0")
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    say(f"2880x5120x3 uint8 frame, crop_border 4, {torch.cuda.get_device_name(0)}; host: {cpus} CPUs visible")
    a = frame(np.random.default_rng(0), 2880, 5120)
    da = torch.from_numpy(a).to(dev)
    opt = {"type": "calculate_niqe", "crop_border": 4, "pris_params": pris}
    for _ in range(2):
        got = calculate_niqe_u8(da, opt)
    per = collections.defaultdict(list)
    for _ in range(args.reps):
        with ops.profile() as rec:
            ops.niqe_stats(da, crop_border=4)
        torch.cuda.synchronize()
        for name, _, s, e, _, _ in rec:
            per[name].append(s.elapsed_time(e) * 1e3)
    say("A. device, median microseconds per launch")
    total = 0.0
    for name, us in per.items():
        total += statistics.median(us)
        say(f"   {name:24s} {statistics.median(us):9.1f} us  (min {min(us):9.1f})")
    s96, s48 = ops.niqe_stats(da, crop_border=4)
    say(f"   all five                 {total:9.1f} us; downloaded: {(s96.numel() + s48.numel()) * 8} bytes of block sums")
    t0 = time.perf_counter()
    want = niqe.calculate_niqe(a, 4, pris_params=pris)
    say(f"B. host niqe.calculate_niqe: {time.perf_counter() - t0:6.2f} s")
    say(f"C. score host {want!r} device {got!r} |d| {abs(got - want):.3e}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
