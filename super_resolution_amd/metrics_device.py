"""PSNR / SSIM of 8-bit frames that are already on the device (`val.metrics_on_device`): hat_u8_metrics delivers the sum of
squared differences and the per-channel SSIM-map sums, `finalize` turns them into the numbers `metrics.calculate_psnr` /
`metrics.calculate_ssim` return for the same uint8 arrays.  Only the sums (32 bytes per sample) come back to the host.
NIQE (`calculate_niqe`, which needs no second frame): ops.niqe_stats delivers 25 sums per block and scale (2 x nblocks x 200
bytes per sample), niqe.features_from_stats / niqe.score finish on the host in fp64.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

DEVICE_METRICS = ("calculate_psnr", "calculate_ssim", "calculate_niqe")   # the `type`s computed here; any other stays with metrics.calculate_metric
PAIRED_METRICS = ("calculate_psnr", "calculate_ssim")                      # those of them that need the second frame

_buffers = {}   # (device, B, h, w, crop_border, y_channel, psnr, ssim) -> (sums, workspace)


def finalize(sums, h: int, w: int, crop_border: int, y_channel: bool) -> dict:
    """sums: the four doubles of one sample (squared-error sum, SSIM-map sum of channel 0, 1, 2) for (h,w,3) frames ->
    {'psnr', 'ssim'} as metrics.calculate_psnr / calculate_ssim define them.  Pure host code."""
    s = np.asarray(sums, dtype=np.float64).reshape(4)
    hc, wc = h - 2 * crop_border, w - 2 * crop_border
    nch = 1 if y_channel else 3
    mse = s[0] / np.float64(hc * wc * nch)
    psnr = float("inf") if mse == 0 else float(10.0 * np.log10(255.0 * 255.0 / mse))
    ssim = float(np.mean([s[1 + c] / np.float64((hc - 10) * (wc - 10)) for c in range(nch)])) if hc > 10 and wc > 10 else float("nan")
    return {"psnr": psnr, "ssim": ssim}


def _buffers_for(dev, B, h, w, crop_border, y_channel, bgr, psnr, ssim):
    key = (dev, B, h, w, crop_border, y_channel, psnr, ssim)
    buf = _buffers.get(key)
    if buf is None:
        need = ops.u8_metrics_workspace_bytes(B, h, w, crop_border=crop_border, y_channel=y_channel, bgr=bgr, psnr=psnr, ssim=ssim)
        buf = _buffers[key] = (torch.zeros(B, 4, dtype=torch.float64, device=dev), torch.zeros(max(need, 8), dtype=torch.uint8, device=dev))
    return buf


def calculate_niqe_u8(a: torch.Tensor, opt: dict, *, bgr: bool = False):
    """a: (h,w,3) or (B,h,w,3) uint8 device tensor; opt: one metric entry of type calculate_niqe ({crop_border[, input_order,
    convert_to, pris_params]}) -> metrics.calculate_niqe of the same uint8 array (a float; a list for B > 1).  Only the block
    sums are downloaded."""
    from . import niqe
    if opt.get("input_order", "HWC") != "HWC":
        raise RuntimeError(f"calculate_niqe on the device scores (h,w,3) frames: input_order {opt['input_order']!r} is not 'HWC'")
    convert_to = opt.get("convert_to", "y")
    if convert_to == "gray":
        raise NotImplementedError("calculate_niqe: convert_to 'gray' is cv2.cvtColor's BGR2GRAY in the reference, whose float "
                                  "arithmetic cannot be pinned without OpenCV; use convert_to 'y'")
    if convert_to != "y":
        raise ValueError(f"calculate_niqe: convert_to is 'y' (or 'gray', unsupported), got {convert_to!r}")
    pris = niqe.pris_params(opt.get("pris_params"))   # before any launch: a missing model is an error of the configuration
    with torch.cuda.device(a.device):
        s96, s48 = ops.niqe_stats(a, crop_border=int(opt["crop_border"]), bgr=bgr)
    h96, h48 = s96.cpu().numpy(), s48.cpu().numpy()
    vals = [niqe.score(niqe.features_from_stats(h96[i], niqe.BLOCK), niqe.features_from_stats(h48[i], niqe.BLOCK // 2), pris)
            for i in range(h96.shape[0])]
    return vals[0] if len(vals) == 1 else vals


def calculate_metrics_u8(a: torch.Tensor, b, metrics_opt: dict, *, bgr: bool = False, niqe: bool = False) -> dict:
    """a, b: (h,w,3) or (B,h,w,3) uint8 device tensors; metrics_opt: the YAML's `val.metrics` ({name: {type, crop_border,
    test_y_channel}}).  Returns {name: value} for every entry of type calculate_psnr / calculate_ssim (a float; a list of
    floats, one per sample, for B > 1); entries of another type are left out.  Entries that share (crop_border,
    test_y_channel) are one launch.  niqe=True (HATModel passes it) also scores the entries of type calculate_niqe, each on
    `a` alone (calculate_niqe_u8); b may then be None when there is no PSNR / SSIM entry.  Without it they are left out like any
    other type, as before NIQE existed here.  The sums and the kernels' workspaces are kept per shape, so a repeated shape
    allocates nothing on the device."""
    paired = any(m.get("type") in PAIRED_METRICS for m in (metrics_opt or {}).values())
    if b is None:
        if paired:
            raise RuntimeError("calculate_metrics_u8: PSNR / SSIM entries need the second frame")
        b = a
    if tuple(a.shape) != tuple(b.shape):
        raise AssertionError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    a4, b4 = (a, b) if a.dim() == 4 else (a.unsqueeze(0), b.unsqueeze(0))
    B, h, w, _ = a4.shape
    groups = {}
    out = {}
    for name, mopt in (metrics_opt or {}).items():
        if mopt.get("type") in PAIRED_METRICS:
            groups.setdefault((int(mopt["crop_border"]), bool(mopt.get("test_y_channel", False))), []).append((name, mopt["type"]))
        elif niqe and mopt.get("type") == "calculate_niqe":
            out[name] = calculate_niqe_u8(a4, mopt, bgr=bgr)
    for (crop, y), entries in groups.items():
        psnr = any(t == "calculate_psnr" for _, t in entries)
        ssim = any(t == "calculate_ssim" for _, t in entries)
        sums, ws = _buffers_for(a4.device, B, h, w, crop, y, bgr, psnr, ssim)
        with torch.cuda.device(a4.device):
            ops.u8_metrics(a4, b4, sums, ws, crop_border=crop, y_channel=y, bgr=bgr, psnr=psnr, ssim=ssim)
        host = sums.cpu().numpy()
        vals = [finalize(host[i], h, w, crop, y) for i in range(B)]
        for name, t in entries:
            k = "psnr" if t == "calculate_psnr" else "ssim"
            out[name] = vals[0][k] if B == 1 else [v[k] for v in vals]
    return {name: out[name] for name in (metrics_opt or {}) if name in out}
