"""tools/resize_path.py — what the device imresize costs and saves at the headline size (a 2880x5120 ground truth -> 720x1280).

    python tools/resize_path.py [--parent-tree /path/to/built/parent/checkout] [--out profiles/r09_resize_path.txt]

Without --section this is a driver that never opens the GPU itself: it runs the sections one after the other as fresh
processes, each under its own `timeout`, and stops at the first one that fails.  Sections:
  A. kernels at 2880x5120 -> 720x1280, f = 4, padded to the window: the two launches under ops.profile(); medians, algorithmic
     bytes, share of the HBM rate, and the bytes a one-launch kernel would save.
  B. host per frame at the same size: resize.imresize_u8 (numpy, this definition) and an evaluation shaped like the
     reference's loop over the same tables (matlab_functions.py:142-169: per output row and channel one Tensor.mv of a
     transposed (P, w) slice of the mirrored image, then per output column one mv of an (oh, P) slice; torch threads as
     printed), against ops.imresize with the 44 MB upload from pageable memory.
  C. nondist_validation per image with ImageNetPairedDataset (a tiny network, so the data path shows): the float route
     against lq_on_device + metrics_on_device, save_img off.
  D. with --parent-tree: `bench.py --gpus 1 --steps 20 --warmup 5` of the parent commit (a built checkout of it) and of this
     build as fresh processes on an otherwise idle card, alternated; the spread between identical parent runs is printed
     beside the difference.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0      # MI355X peak HBM rate, TB/s
LIMITS = {"A": 240, "B": 420, "C": 420}      # seconds per section
H, W, F = 2880, 5120, 4
med = statistics.median


def say(s=""):
    print(s, flush=True)


def _sizes():
    oh, ow = H // F, W // F
    return oh, ow, -(-oh // 16) * 16, -(-ow // 16) * 16


def section_a(args):
    import numpy as np
    import torch
    from super_resolution_amd import ops
    dev = torch.device("cuda:0")
    oh, ow, Hp, Wp = _sizes()
    say(f"A. kernels: imresize {H}x{W} uint8 -> {oh}x{ow} fp32 planes padded to {Hp}x{Wp}, {torch.cuda.get_device_name(0)}")
    gt = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8))[None].to(dev)
    dst = torch.empty(1, 3, Hp, Wp, device=dev)
    for _ in range(3):
        ops.imresize(gt, 1 / F, dst=dst, pad_to=(Hp, Wp))
    torch.cuda.synchronize()
    with ops.profile() as rec:
        for _ in range(args.launches):
            ops.imresize(gt, 1 / F, dst=dst, pad_to=(Hp, Wp))
    torch.cuda.synchronize()
    per = {}
    for name, _, s_, e_, tag, nbytes in rec:
        per.setdefault(name, ([], nbytes))[0].append(s_.elapsed_time(e_) * 1e3)
    tot = 0.0
    for name, (v, nbytes) in per.items():
        m = med(v)
        tot += m
        say(f"   {name:30s} median of {len(v)}: {m:8.1f} us  min {min(v):.1f} max {max(v):.1f}; {nbytes / 1e6:.1f} MB algorithmic -> "
            f"{nbytes / m / 1e6:.2f} TB/s = {nbytes / m / 1e6 / HBM_TBS * 100:.0f} % of {HBM_TBS:.0f} TB/s")
    say(f"   both launches (medians added) {tot:.1f} us; one launch that kept the intermediate on chip would move "
        f"{3 * (H * W + 4 * Hp * Wp) / 1e6:.1f} MB instead of {3 * (H * W + 8 * oh * W + 4 * Hp * Wp) / 1e6:.1f} MB")
    return 0


def reference_shaped(x, w_h, s_h, w_w, s_w):
    """The reference's loop shape over this build's tables: x (3,h,w) torch fp32 -> (3,oh,ow)."""
    import torch
    P_h, P_w = w_h.shape[1], w_w.shape[1]
    oh, ow = w_h.shape[0], w_w.shape[0]
    wh, ww = torch.from_numpy(w_h), torch.from_numpy(w_w)
    sh, sw = torch.from_numpy(s_h).long(), torch.from_numpy(s_w).long()
    out1 = torch.empty(3, oh, x.shape[2])
    for i in range(oh):
        rows = x[:, sh[i], :]                                   # the P mirrored rows (the reference slices its augmented copy)
        for c in range(3):
            out1[c, i, :] = rows[c].transpose(0, 1).mv(wh[i])
    out2 = torch.empty(3, oh, ow)
    for j in range(ow):
        cols = out1[:, :, sw[j]]
        for c in range(3):
            out2[c, :, j] = cols[c].mv(ww[j])
    return out2


def section_b(args):
    import numpy as np
    import torch
    from super_resolution_amd import ops, resize as R
    dev = torch.device("cuda:0")
    oh, ow, Hp, Wp = _sizes()
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    torch.set_num_threads(min(16, cpus))
    say(f"B. host per frame (ms) at {H}x{W} -> {oh}x{ow}; CPUs visible {cpus}, torch threads {torch.get_num_threads()}")
    gt_host = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    w_h, s_h = R.weights_indices(H, oh, 1 / F)
    w_w, s_w = R.weights_indices(W, ow, 1 / F)
    d = torch.empty(1, 3, Hp, Wp, device=dev)
    ops.imresize(torch.from_numpy(gt_host)[None].to(dev), 1 / F, dst=d, pad_to=(Hp, Wp))      # tables, code objects
    torch.cuda.synchronize()
    t_def, t_ref, t_dev = [], [], []
    for _ in range(args.host_frames):
        t0 = time.perf_counter()
        ref = R.imresize_u8(gt_host, 1 / F)
        t1 = time.perf_counter()
        y = reference_shaped(torch.from_numpy(R.u8_planes(gt_host)), w_h, s_h, w_w, s_w)
        t2 = time.perf_counter()
        ops.imresize(torch.from_numpy(gt_host)[None].to(dev), 1 / F, dst=d, pad_to=(Hp, Wp))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_def.append((t1 - t0) * 1e3)
        t_ref.append((t2 - t1) * 1e3)
        t_dev.append((t3 - t2) * 1e3)
    say(f"   resize.imresize_u8 (numpy, the definition):                 median {med(t_def):.1f}  ({' '.join(f'{v:.0f}' for v in t_def)})")
    say(f"   /255 + the reference-shaped loop of Tensor.mv calls:        median {med(t_ref):.1f}  ({' '.join(f'{v:.0f}' for v in t_ref)}); "
        f"max |loop - definition| {float(np.abs(y.numpy() - ref).max()):.2e}")
    say(f"   upload {H * W * 3 / 1e6:.1f} MB (pageable) + the two launches + synchronise: median {med(t_dev):.1f}  ({' '.join(f'{v:.1f}' for v in t_dev)})")
    say(f"   device result == definition: {bool(np.array_equal(d.cpu().numpy()[0, :, :oh, :ow], ref))}")
    return 0


def section_c(args):
    import numpy as np
    import torch
    from oracle import hat_oracle as O
    from super_resolution_amd import data as D, synth
    from super_resolution_amd.models import HATModel
    say("C. nondist_validation per image (ms), ImageNetPairedDataset, 4 GT images 1024x1536, x4, tiny network, save_img off")
    netopt = dict(type="HAT", upscale=4, in_chans=3, img_size=32, window_size=16, compress_ratio=4, squeeze_factor=4, conv_scale=0.01,
                  overlap_ratio=0.5, img_range=1.0, depths=[2], embed_dim=24, num_heads=[2], mlp_ratio=2, upsampler="pixelshuffle",
                  resi_connection="1conv", compute_dtype="bf16")
    metrics = {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": True},
               "ssim": {"type": "calculate_ssim", "crop_border": 4, "test_y_channel": True}}
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(1)
        for i in range(4):
            D.write_image(rng.integers(0, 256, (1024, 1536, 3), dtype=np.uint8), os.path.join(tmp, "gt", f"im{i}.png"))
        cfg = O.make_cfg(**{k: v for k, v in netopt.items() if k not in ("type", "compute_dtype")})
        torch.save({"params": synth.synth_state_dict(O.blank_state_dict(cfg), 21)}, os.path.join(tmp, "net.pth"))
        ds = lambda: D.FolderDataset({"name": "Toy", "type": "ImageNetPairedDataset", "dataroot_gt": os.path.join(tmp, "gt"), "scale": 4, "phase": "test"})
        for label, val in (("float route (host LQ, host metrics)", {}), ("lq_on_device + metrics_on_device", {"lq_on_device": True, "metrics_on_device": True})):
            m = HATModel({"name": "toy", "scale": 4, "network_g": dict(netopt), "path": {"pretrain_network_g": os.path.join(tmp, "net.pth")},
                          "val": dict({"metrics": metrics}, **val)}, device="cuda:0")
            m.nondist_validation(ds(), save_img=False)                  # warm-up: packs, workspaces, tables
            ts = []
            for _ in range(2):
                t0 = time.perf_counter()
                mean, _ = m.nondist_validation(ds(), save_img=False)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / 4)
            say(f"   {label:40s} {min(ts):.1f} per image (runs {' '.join(f'{v:.1f}' for v in ts)})  psnr {mean['psnr']:.6f} ssim {mean['ssim']:.8f}")
    return 0


def section_d(parent_tree, lines):
    def out(s):
        say(s)
        lines.append(s)
    out("D. bench.py --gpus 1 --steps 20 --warmup 5, fresh processes alternated")
    runs = {"parent": [], "branch": []}
    for _ in range(3):
        for side, tree in (("parent", os.path.abspath(parent_tree)), ("branch", ROOT)):
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20",
                                "--warmup", "5"], capture_output=True, text=True, cwd=tree)
            if r.returncode != 0:
                out(f"   bench.py ({side}) failed with {r.returncode}: {r.stderr[-400:]}")
                return 1
            runs[side].append(json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1]))
    out(f"   result keys: {sorted(runs['parent'][0])}")
    for side in ("parent", "branch"):
        out(f"   {side}: " + " | ".join(json.dumps({k: v for k, v in r.items() if isinstance(v, (int, float))}) for r in runs[side]))
    key = next((k for k in ("ms_per_step", "step_ms", "latency_ms", "ms") if k in runs["parent"][0]), None)
    if key:
        pv, bv = [r[key] for r in runs["parent"]], [r[key] for r in runs["branch"]]
        out(f"   {key}: parent {' '.join(f'{v:.3f}' for v in pv)} | this build {' '.join(f'{v:.3f}' for v in bv)}")
        out(f"   spread of identical parent runs {max(pv) - min(pv):.3f}; this build - parent (medians) = {med(bv) - med(pv):+.3f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["A", "B", "C"], default=None, help="run one section in this process (the driver does that)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.section:
        return {"A": section_a, "B": section_b, "C": section_c}[args.section](args)
    lines, rc = [], 0

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for sec in ("A", "B", "C"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[sec]), sys.executable, os.path.abspath(__file__), "--section", sec, "--launches",
                            str(args.launches), "--host-frames", str(args.host_frames)], capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines.extend(r.stdout.splitlines())
        flush()
        if r.returncode != 0:
            say(f"section {sec} ended with {r.returncode}: {r.stderr[-600:]}")
            return 1
    if args.parent_tree:
        rc = section_d(args.parent_tree, lines)
    flush()
    return rc


if __name__ == "__main__":
    sys.exit(main())
