#!/usr/bin/env python3
"""Golden vectors for ESCFP, made by running THE REFERENCE ITSELF (`hat.archs.esc_fp_arch.ESCFP`, attn_type='Naive', imported with
gen_golden.py's loader shim; build container only).  Data only: weights are regenerated from the seed (tests/escfp_ref.py's
escfp_state_dict: every parameter randomised — lk_channel, lk_spatial and plk.proj.3 too, a zero proj.3 would hide the dynamic
kernel — the relative-position bias at std 0.5) and never stored.  Writes NEW files only.

  escfp_a   n_blocks 1, conv_blocks 1, exp_ratio 1.25, x2 on 1x3x40x72: both pads 24; hidden widths 72 (Block.proj) and 60
  escfp_b   n_blocks 2, conv_blocks 2, exp_ratio 2, x4 on 1x3x33x64: pad 31 (the largest reflect allows) and no pad; hidden 96
  escfp_c   n_blocks 1, conv_blocks 1, exp_ratio 1.25, x3 on a batch of two different 33x40 images: per-sample dynamic kernels,
            the odd bicubic phase
  escfp_d   case a's x2 checkpoint loaded into a x4 model on 33x40: pins the to_img conversion of load_state_dict
Each file: x, y and (a, b, c) the stream after the first ConvFFN, the attention and the first conv block at esc_ref.tap_pixels
(of every sample).  escfp_surface.json: keys and shapes of the cases and of ESC_FP_X2 / X3 / X4, and per case the reference's own
bf16 deviation (net.bfloat16() on the bf16 input against its fp32 output: PSNR at peak 1 and max-abs).

    python tests/golden/gen_golden_escfp.py
"""
from __future__ import annotations

import importlib
import json
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import import_reference  # noqa: E402
from gen_golden_esc import psnr, surface, taps_of  # noqa: E402
import escfp_ref as R  # noqa: E402
from super_resolution_amd import synth  # noqa: E402


def bf16_deviation(ESCFP, cfg, sd, x, y):
    net = ESCFP(**cfg, attn_type="Naive").eval()
    net.load_state_dict(sd, strict=True)
    yb = net.bfloat16()(x.bfloat16()).float()
    return dict(psnr=psnr(yb, y), max_abs=float((yb - y).abs().max()))


def main():
    torch.set_num_threads(4)
    import_reference()
    sys.modules["basicsr.utils"].get_root_logger = lambda: logging.getLogger("escfp")
    importlib.import_module("hat.archs.esc_fp_arch")
    ESCFP = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("ESCFP")
    meta = {"w_seed": R.W_SEED, "x_seed": R.X_SEED, "cases": {}, "surfaces": {}, "nparams": {}}
    with torch.no_grad():
        for name, cfg in R.SURFACE_CFGS.items():
            net = ESCFP(**cfg, attn_type="Naive")
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net))
            meta["nparams"][name] = sum(p.numel() for p in net.parameters())
        sds = {}
        for name, (cfg, frame) in R.CASES.items():
            net = ESCFP(**cfg, attn_type="Naive").eval()
            sd = sds[name] = R.escfp_state_dict(net.state_dict(), R.W_SEED)
            net.load_state_dict(sd, strict=True)
            x = synth.synth_input(R.X_SEED, frame)
            y, got = taps_of(net, x)
            px = R.tap_pixels(frame[2], frame[3])
            arrays = {k: got[k].reshape(frame[0], 48, -1)[:, :, px].permute(0, 2, 1).contiguous().numpy() for k in R.TAPS}   # (B, pixels, 48)
            np.savez(f"{HERE}/escfp_{name}.npz", x=x.numpy(), y=y.numpy(), tap_pixels=px, **arrays)
            meta["cases"][name] = dict(cfg=cfg, frame=list(frame), surface=surface(net), nparams=sum(p.numel() for p in net.parameters()),
                                       bf16=bf16_deviation(ESCFP, cfg, sd, x, y))
            if frame[0] > 1:   # the batch against its samples one at a time, in the reference
                meta["cases"][name]["batch_vs_single_max_abs"] = max(float((net(x[b:b + 1]) - y[b:b + 1]).abs().max()) for b in range(frame[0]))
        cfg_d, frame_d = R.CASE_D
        net = ESCFP(**cfg_d, attn_type="Naive").eval()
        net.load_state_dict(sds["a"], strict=True)
        x = synth.synth_input(R.X_SEED, frame_d)
        y = net(x)
        np.savez(f"{HERE}/escfp_d.npz", x=x.numpy(), y=y.numpy())
        meta["cases"]["d"] = dict(cfg=cfg_d, frame=list(frame_d), surface=meta["cases"]["a"]["surface"], loaded_from="a",
                                  nparams=meta["cases"]["a"]["nparams"], bf16=bf16_deviation(ESCFP, cfg_d, sds["a"], x, y))
    with open(f"{HERE}/escfp_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))


if __name__ == "__main__":
    main()
