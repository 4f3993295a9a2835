"""tools/metrics_path.py — what scoring on the device costs and saves on the headline config (HAT-S x4, 720x1280 in, bf16).

    timeout -k 10 1100 python tools/metrics_path.py [--images 3] [--out profiles/r07_metrics_path.txt]

One process, steps in order, the first failure ends the run.  Reported, for 2880x5120 frames and crop_border 4:
  A. device time of hat_u8_metrics (PSNR + SSIM in one launch) for Y and for RGB under ops.profile(), and the difference
     to the host's numbers on the same pair;
  B. metrics.calculate_psnr + calculate_ssim on the host for the same pair, in this process (CPU count printed);
  C. wall time per image of HATModel.nondist_validation over --images synthetic 720p images with 8-bit ground truth, three
     ways (host metrics on the float route, val.u8_on_device, val.metrics_on_device), with save_img on and off.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HATS = dict(type="HAT", upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01,
            overlap_ratio=0.5, img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2,
            upsampler="pixelshuffle", resi_connection="1conv", compute_dtype="bf16")
METRICS = {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": True},
           "ssim": {"type": "calculate_ssim", "crop_border": 4, "test_y_channel": True}}


def smooth_pair(rng, h, w):
    """a blocky smooth image and itself plus noise of sigma 4 (the shape of an SR result against its ground truth)"""
    import numpy as np
    low = rng.integers(30, 226, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    a = np.repeat(np.repeat(low, 8, axis=0), 8, axis=1)[:h, :w]
    b = np.clip(np.round(a + rng.normal(0.0, 4.0, a.shape).astype(np.float32)), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from super_resolution_amd import data as D, metrics as M, ops, synth
    from super_resolution_amd.metrics_device import finalize
    from super_resolution_amd.models import HATModel
    from super_resolution_amd.registry import build_network
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    say(f"2880x5120x3 uint8 pairs, crop_border 4, {torch.cuda.get_device_name(0)}; host: {cpus} CPUs visible, {torch.get_num_threads()} torch threads")
    rng = np.random.default_rng(0)
    a, b = smooth_pair(rng, 2880, 5120)
    da, db = torch.from_numpy(a)[None].to(dev), torch.from_numpy(b)[None].to(dev)
    sums = torch.zeros(1, 4, dtype=torch.float64, device=dev)
    # ---- A + B
    say("A/B. hat_u8_metrics (PSNR + SSIM, one launch + the fixed-order finish) against metrics.calculate_psnr + calculate_ssim")
    for y in (True, False):
        ws = torch.empty(ops.u8_metrics_workspace_bytes(1, 2880, 5120, crop_border=4, y_channel=y), dtype=torch.uint8, device=dev)
        for _ in range(3):
            ops.u8_metrics(da, db, sums, ws, crop_border=4, y_channel=y)
        with ops.profile() as rec:
            for _ in range(args.reps):
                ops.u8_metrics(da, db, sums, ws, crop_border=4, y_channel=y)
        torch.cuda.synchronize()
        us = sorted(s.elapsed_time(e) * 1e3 for _, _, s, e, _, _ in rec)
        got = finalize(sums.cpu().numpy()[0], 2880, 5120, 4, y)
        t0 = time.perf_counter()
        psnr = M.calculate_psnr(a, b, 4, test_y_channel=y)
        t1 = time.perf_counter()
        ssim = M.calculate_ssim(a, b, 4, test_y_channel=y)
        t2 = time.perf_counter()
        nch = 1 if y else 3
        fma = nch * 2870 * 5110 * 5 * 22
        say(f"   {'Y  ' if y else 'RGB'} device: median {statistics.median(us):9.1f} us  min {us[0]:9.1f} us  ({rec[0][0]}; {2 * 2880 * 5120 * 3 / 1e6:.0f} MB read, "
            f"{fma / 1e9:.2f} G fp64 multiply-adds in the filters -> {fma / statistics.median(us) / 1e6:.2f} T/s; workspace {ws.numel()} bytes)")
        say(f"       host:   calculate_psnr {t1 - t0:6.2f} s  calculate_ssim {t2 - t1:6.2f} s")
        say(f"       psnr host {psnr!r} device {got['psnr']!r} |d| {abs(got['psnr'] - psnr):.3e} dB   ssim host {ssim!r} device {got['ssim']!r} |d| {abs(got['ssim'] - ssim):.3e}")
    del da, db
    # ---- C
    say(f"C. HATModel.nondist_validation, wall seconds per image over {args.images} 720x1280 images (8-bit ground truth 2880x5120), metrics: "
        "PSNR + SSIM on Y, crop_border 4")
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.images):
            gt, _ = smooth_pair(np.random.default_rng(10 + i), 2880, 5120)
            D.write_image(gt, os.path.join(tmp, "gt", f"im{i}.png"))
            D.write_image(np.ascontiguousarray(gt[::4, ::4]), os.path.join(tmp, "lq", f"im{i}.png"))
        net = build_network(dict(HATS)).eval()
        torch.save({"params": synth.synth_state_dict(net.state_dict(), 1234)}, os.path.join(tmp, "net.pth"))
        del net
        ds = D.FolderDataset({"name": "P", "type": "PairedImageDataset", "dataroot_gt": os.path.join(tmp, "gt"), "dataroot_lq": os.path.join(tmp, "lq"),
                              "scale": 4, "phase": "test"})
        results = {}
        for label, val in (("host metrics (float route)", {}), ("val.u8_on_device", {"u8_on_device": True}),
                           ("val.metrics_on_device", {"metrics_on_device": True})):
            opt = {"name": "p", "scale": 4, "network_g": dict(HATS), "path": {"visualization": os.path.join(tmp, "vis"), "pretrain_network_g": os.path.join(tmp, "net.pth")},
                   "val": dict({"suffix": None, "metrics": METRICS}, **val)}
            model = HATModel(opt, device=str(dev))
            with torch.no_grad():                    # warm-up: the engine packs its weights and workspaces on the first call
                model.get_bare_model(model.net_g)(torch.zeros(1, 3, 720, 1280, device=dev))
                model.get_bare_model(model.net_g).forward_u8(torch.zeros(1, 720, 1280, 3, dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            row = []
            for save in (True, False):
                t0 = time.perf_counter()
                mean, _ = model.nondist_validation(ds, save_img=save)
                torch.cuda.synchronize()
                row.append((time.perf_counter() - t0) / max(args.images, 1))
                results[(label, save)] = mean
            say(f"   {label:28s} save_img on {row[0]:7.2f} s   save_img off {row[1]:7.2f} s   psnr {mean['psnr']:.4f} ssim {mean['ssim']:.4f}")
            del model
        ref = results[("val.u8_on_device", True)]
        got = results[("val.metrics_on_device", True)]
        say(f"   metrics_on_device against u8_on_device, dataset means: |dPSNR| {abs(got['psnr'] - ref['psnr']):.3e} dB  |dSSIM| {abs(got['ssim'] - ref['ssim']):.3e}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
