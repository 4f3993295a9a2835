#!/usr/bin/env python3
"""Golden vectors for ESC, made by running THE REFERENCE ITSELF (`hat.archs.esc_arch.ESC`, attn_type='Naive', imported with
gen_golden.py's loader shim; build container only).  Data only: weights are regenerated from the seed (tests/esc_ref.py's
esc_state_dict: every parameter randomised, the relative-position bias at std 0.5) and never stored.  Writes NEW files only.

  esc_a   n_blocks 1, conv_blocks 1, exp_ratio 1.25, x2 on 40x72: neither side a multiple of 32 (pads 24 and 24), 2 x 3 windows
  esc_b   n_blocks 2, conv_blocks 2, exp_ratio 2, use_ln, x4 on 33x64: pad 31 (the largest reflect allows) and no pad
  esc_c   case a after convert(): the same output from the baked filter
  esc_d   case a's x2 checkpoint loaded into a x3 model on 33x40: pins the to_img conversion of load_state_dict
Each file: x, y and (a, b) the stream after the first ConvFFN, the attention and the first conv block at esc_ref.tap_pixels.
esc_surface.json: keys and shapes of the cases and of the ESC, ESC-light and ESCReal-body configs, and per case the reference's
own bf16 deviation (net.bfloat16() on the bf16 input against its fp32 output: PSNR at peak 1 and max-abs).

    python tests/golden/gen_golden_esc.py
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
import esc_ref  # noqa: E402
from super_resolution_amd import synth  # noqa: E402


def surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def bf16_deviation(ESC, cfg, sd, x, y):
    net = ESC(**cfg, attn_type="Naive").eval()
    net.load_state_dict(sd, strict=True)
    yb = net.bfloat16()(x.bfloat16()).float()
    return dict(psnr=psnr(yb, y), max_abs=float((yb - y).abs().max()))


def taps_of(net, x):
    """The stream inside the first Block, by hooks on the reference's own modules."""
    got, blk = {}, net.blocks[0]
    hs = [blk.proj.register_forward_hook(lambda m, i, o: got.__setitem__("ffn0", o.clone())),
          blk.attn.register_forward_hook(lambda m, i, o: got.__setitem__("attn0", got["ffn0"] + o)),
          blk.pconvs[0].register_forward_hook(lambda m, i, o: got.__setitem__("conv0", got["attn0"] + o))]
    y = net(x)
    for h in hs:
        h.remove()
    return y, got


def main():
    torch.set_num_threads(4)
    import_reference()
    sys.modules["basicsr.utils"].get_root_logger = lambda: logging.getLogger("esc")
    importlib.import_module("hat.archs.esc_arch")
    ESC = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("ESC")
    meta = {"w_seed": esc_ref.W_SEED, "x_seed": esc_ref.X_SEED, "cases": {}, "surfaces": {}, "nparams": {}}
    with torch.no_grad():
        for name, cfg in esc_ref.SURFACE_CFGS.items():
            net = ESC(**cfg, attn_type="Naive")
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net))
            meta["nparams"][name] = sum(p.numel() for p in net.parameters())
        sds = {}
        for name, (cfg, frame) in esc_ref.CASES.items():
            net = ESC(**cfg, attn_type="Naive").eval()
            sd = sds[name] = esc_ref.esc_state_dict(net.state_dict(), esc_ref.W_SEED)
            net.load_state_dict(sd, strict=True)
            x = synth.synth_input(esc_ref.X_SEED, frame)
            y, got = taps_of(net, x)
            px = esc_ref.tap_pixels(frame[2], frame[3])
            arrays = {k: got[k][0].reshape(64, -1)[:, px].t().contiguous().numpy() for k in esc_ref.TAPS}
            np.savez(f"{HERE}/esc_{name}.npz", x=x.numpy(), y=y.numpy(), tap_pixels=px, **arrays)
            meta["cases"][name] = dict(cfg=cfg, frame=list(frame), surface=surface(net), nparams=sum(p.numel() for p in net.parameters()),
                                       bf16=bf16_deviation(ESC, cfg, sd, x, y))
            if name == "a":
                net.convert()
                yc = net(x)
                np.savez(f"{HERE}/esc_c.npz", x=x.numpy(), y=yc.numpy())
                meta["cases"]["c"] = dict(meta["cases"]["a"], converted_max_abs_vs_a=float((yc - y).abs().max()))
        cfg_d, frame_d = dict(esc_ref.CASES["a"][0], upscaling_factor=3), (1, 3, 33, 40)
        net = ESC(**cfg_d, attn_type="Naive").eval()
        net.load_state_dict(sds["a"], strict=True)
        x = synth.synth_input(esc_ref.X_SEED, frame_d)
        y = net(x)
        np.savez(f"{HERE}/esc_d.npz", x=x.numpy(), y=y.numpy())
        meta["cases"]["d"] = dict(cfg=cfg_d, frame=list(frame_d), surface=meta["cases"]["a"]["surface"], loaded_from="a",
                                  nparams=meta["cases"]["a"]["nparams"], bf16=bf16_deviation(ESC, cfg_d, sds["a"], x, y))
    with open(f"{HERE}/esc_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))


if __name__ == "__main__":
    main()
