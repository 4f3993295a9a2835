"""PSNR / SSIM of 8-bit frames that are already on the device (`val.metrics_on_device`): hat_u8_metrics delivers the sum of
squared differences and the per-channel SSIM-map sums, `finalize` turns them into the numbers `metrics.calculate_psnr` /
`metrics.calculate_ssim` return for the same uint8 arrays.  Only the sums (32 bytes per sample) come back to the host.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

DEVICE_METRICS = ("calculate_psnr", "calculate_ssim")   # the `type`s computed here; any other stays with metrics.calculate_metric

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


def calculate_metrics_u8(a: torch.Tensor, b: torch.Tensor, metrics_opt: dict, *, bgr: bool = False) -> dict:
    """a, b: (h,w,3) or (B,h,w,3) uint8 device tensors; metrics_opt: the YAML's `val.metrics` ({name: {type, crop_border,
    test_y_channel}}).  Returns {name: value} for every entry of type calculate_psnr / calculate_ssim (a float; a list of
    floats, one per sample, for B > 1); entries of another type are left out.  Entries that share (crop_border,
    test_y_channel) are one launch.  The sums and the kernel's workspace are kept per shape, so a repeated shape allocates
    nothing on the device."""
    if tuple(a.shape) != tuple(b.shape):
        raise AssertionError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    a4, b4 = (a, b) if a.dim() == 4 else (a.unsqueeze(0), b.unsqueeze(0))
    B, h, w, _ = a4.shape
    groups = {}
    for name, mopt in (metrics_opt or {}).items():
        if mopt.get("type") in DEVICE_METRICS:
            groups.setdefault((int(mopt["crop_border"]), bool(mopt.get("test_y_channel", False))), []).append((name, mopt["type"]))
    out = {}
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
