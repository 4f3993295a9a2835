#!/usr/bin/env python3
"""Golden vectors for ESCReal, made by running THE REFERENCE ITSELF (`hat.archs.esc_real_arch.ESCReal`, attn_type='Naive', imported
with gen_golden.py's loader shim; build container only).  Data only: weights are regenerated from the seed (tests/escreal_ref.py's
escreal_state_dict: esc_ref.esc_state_dict for the body, skip.* and the heads randomised, DySample's offset / scope weights at std
0.3 so that sampling positions move by more than two pixels and reach the border clamp on every side — asserted below) and never
stored.  Writes NEW files only.

  escreal_a   default head, exp_ratio 2, 33x40: odd sides, reflect pad 31, several tiles, all four borders of the 7x7 reflect
  escreal_b   default head, 2 blocks / 2 conv blocks, exp_ratio 1.25, upscaling_factor=2, 40x72: the output is x4 all the same
  escreal_c   DySample x4 on 33x40          escreal_d   DySample x3 on 33x40          escreal_e   DySample x2 on 40x72
Each file: x, y; a, c, d, e also skip(x) and to_img's input at esc_ref.tap_pixels (160 rows of 64 channels: the kernel tests
lay the feat rows out as a 10 x 16 map, which is as good an input of to_img as any).  escreal_surface.json: keys and shapes of the cases and of the full ESC_Real_X4 config with both heads
(init_pos values included), and per case the reference's own bf16 deviation (net.bfloat16() on the bf16 input against its fp32
output: PSNR at peak 1 and max-abs; null where it is not finite).

On a machine without a GPU DySample.forward's torch.tensor(..., pin_memory=True) raises: torch.tensor is wrapped to drop that
keyword while the reference runs.  The reference is not edited.

    python tests/golden/gen_golden_escreal.py
"""
from __future__ import annotations

import importlib
import json
import logging
import math
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
import escreal_ref  # noqa: E402
from super_resolution_amd import synth  # noqa: E402


def surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def finite_or_none(v):
    return v if math.isfinite(v) else None


def bf16_deviation(ESCReal, cfg, sd, x, y):
    net = ESCReal(**cfg, attn_type="Naive").eval()
    net.load_state_dict(sd, strict=True)
    yb = net.bfloat16()(x.bfloat16()).float()
    p, m = psnr(yb, y), float((yb - y).abs().max())
    if not (math.isfinite(p) and math.isfinite(m)):
        return None
    return dict(psnr=p, max_abs=m)


def taps_of(net, x):
    got = {}
    hs = [net.skip.register_forward_hook(lambda m, i, o: got.__setitem__("skip", o.clone())),
          net.to_img.register_forward_hook(lambda m, i, o: got.__setitem__("feat", i[0].clone()))]
    y = net(x)
    for h in hs:
        h.remove()
    return y, got


def main():
    torch.set_num_threads(4)
    import_reference()
    sys.modules["basicsr.utils"].get_root_logger = lambda: logging.getLogger("esc")
    importlib.import_module("hat.archs.esc_real_arch")
    ESCReal = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("ESCReal")
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "pin_memory"})
    meta = {"w_seed": esc_ref.W_SEED, "x_seed": esc_ref.X_SEED, "cases": {}, "surfaces": {}, "nparams": {}}
    with torch.no_grad():
        for name, cfg in escreal_ref.SURFACE_CFGS.items():
            net = ESCReal(**cfg, attn_type="Naive")
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net))
            meta["nparams"][name] = sum(p.numel() for p in net.parameters())
            if cfg.get("use_dysample"):
                meta["surfaces"][name]["init_pos"] = net.to_img.init_pos.reshape(-1).tolist()
        for name, (cfg, frame) in escreal_ref.CASES.items():
            net = ESCReal(**cfg, attn_type="Naive").eval()
            sd = escreal_ref.escreal_state_dict(net.state_dict(), esc_ref.W_SEED)
            if cfg.get("use_dysample"):
                assert torch.equal(sd["to_img.init_pos"], net.to_img.init_pos), "escreal_ref.init_pos differs from the reference's"
            net.load_state_dict(sd, strict=True)
            x = synth.synth_input(esc_ref.X_SEED, frame)
            y, got = taps_of(net, x)
            assert torch.isfinite(y).all()
            arrays = {}
            if name in escreal_ref.TAP_CASES:
                px = esc_ref.tap_pixels(frame[2], frame[3])
                arrays = dict(tap_pixels=px, skip=escreal_ref.rows_at(got["skip"], px).numpy(), feat=escreal_ref.rows_at(got["feat"], px).numpy())
            case = dict(cfg=cfg, frame=list(frame), out=list(y.shape), surface=surface(net), nparams=sum(p.numel() for p in net.parameters()),
                        bf16=bf16_deviation(ESCReal, cfg, sd, x, y))
            if cfg.get("use_dysample"):
                case["init_pos"] = net.to_img.init_pos.reshape(-1).tolist()
                s = cfg["upscaling_factor"]
                pxs, pys = escreal_ref.dys_positions(got["feat"].double(), esc_ref.d64(sd), s)
                H, W = frame[2], frame[3]
                lo = pxs - (torch.arange(s * W).div(s, rounding_mode="floor"))[None, None, :]
                clamped = dict(left=int((pxs < 0).sum()), right=int((pxs > W - 1).sum()), top=int((pys < 0).sum()), bottom=int((pys > H - 1).sum()))
                assert all(v > 0 for v in clamped.values()), clamped
                case["clamped"] = clamped
                case["max_move"] = float(lo.abs().max())
                assert case["max_move"] > 2.0, case["max_move"]
            np.savez_compressed(f"{HERE}/escreal_{name}.npz", x=x.numpy(), y=y.numpy(), **arrays)
            meta["cases"][name] = case
    torch.tensor = real_tensor
    with open(f"{HERE}/escreal_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg", "init_pos")} for k, v in meta["cases"].items()}, indent=1))
    for name in escreal_ref.CASES:
        print(name, os.path.getsize(f"{HERE}/escreal_{name}.npz"))


if __name__ == "__main__":
    main()
