#!/usr/bin/env python3
"""Golden vectors for ESCRealM, made by running THE REFERENCE ITSELF (`hat.archs.esc_real_arch.ESCRealM`, attn_type='Naive', imported
with gen_golden.py's loader shim; build container only).  Data only: weights are regenerated from the seed
(tests/escrealm_ref.py's escrealm_state_dict; DySample's offset / scope weights at std 0.3 so that sampling clamps on all four
sides — asserted below) and never stored.  Writes NEW files only.

  escrealm_a   x2, unshuffle f=2, nearest+conv, 67x81: both reflect pads of check_img_size live; the body is 34x41
  escrealm_b   x1, unshuffle f=4, pixelshuffledirect, 66x83: pads of 2 and 1, the 48-channel stem
  escrealm_c   x3, plain stem, nearest+conv, 33x40          escrealm_d   x3, pixelshuffle, mid 48, 33x40
  escrealm_e   x4, unshuffle_mod=False, pixelshuffle, mid 48, 2 blocks / 2 conv blocks, exp_ratio 1.25, 33x40
  escrealm_f   x2, unshuffle f=2, dysample, mid 48, 67x81   escrealm_g   upscaling_factor=1, unshuffle_mod=False, conv, 33x40
Each file: x, y; a, b, c, f also skip(x) and to_img's input at esc_ref.tap_pixels of the body's frame.  escrealm_surface.json: keys,
shapes and MetaUpsample values of the cases and of the ESC_Real_X4-sized config with each of the five heads, and per case the
reference's own bf16 deviation (net.bfloat16() on the bf16 input against its fp32 output: PSNR at peak 1 and max-abs).

On a machine without a GPU DySample.forward's torch.tensor(..., pin_memory=True) raises: torch.tensor is wrapped to drop that
keyword while the reference runs.  The reference is not edited.

    python tests/golden/gen_golden_escrealm.py
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
from gen_golden_escreal import bf16_deviation, surface, taps_of  # noqa: E402
import esc_ref  # noqa: E402
import escreal_ref  # noqa: E402
import escrealm_ref  # noqa: E402
from super_resolution_amd import synth  # noqa: E402


def main():
    torch.set_num_threads(4)
    import_reference()
    sys.modules["basicsr.utils"].get_root_logger = lambda: logging.getLogger("esc")
    importlib.import_module("hat.archs.esc_real_arch")
    ESCRealM = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("ESCRealM")
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "pin_memory"})
    meta = {"w_seed": esc_ref.W_SEED, "x_seed": esc_ref.X_SEED, "cases": {}, "surfaces": {}, "nparams": {}}
    with torch.no_grad():
        for name, cfg in escrealm_ref.SURFACE_CFGS.items():
            net = ESCRealM(**cfg, attn_type="Naive")
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net), meta_upsample=net.to_img.MetaUpsample.tolist())
            meta["nparams"][name] = sum(p.numel() for p in net.parameters())
        for name, (cfg, frame) in escrealm_ref.CASES.items():
            net = ESCRealM(**cfg, attn_type="Naive").eval()
            assert net.to_img.MetaUpsample.tolist() == escrealm_ref.meta_upsample(cfg)
            sd = escrealm_ref.escrealm_state_dict(net.state_dict(), cfg, esc_ref.W_SEED)
            for k in sd:
                if k.endswith("init_pos"):
                    assert torch.equal(sd[k], net.state_dict()[k]), "escreal_ref.init_pos differs from the reference's"
            net.load_state_dict(dict(sd), strict=True)
            x = synth.synth_input(esc_ref.X_SEED, frame)
            y, got = taps_of(net, x)
            assert torch.isfinite(y).all()
            f, S = escrealm_ref.stem_of(cfg)
            H, W = got["feat"].shape[-2:]
            arrays = {}
            if name in escrealm_ref.TAP_CASES:
                px = esc_ref.tap_pixels(H, W)
                arrays = dict(tap_pixels=px, skip=escreal_ref.rows_at(got["skip"], px).numpy(), feat=escreal_ref.rows_at(got["feat"], px).numpy())
            case = dict(cfg=cfg, frame=list(frame), body=[H, W], out=list(y.shape), surface=surface(net),
                        meta_upsample=net.to_img.MetaUpsample.tolist(), nparams=sum(p.numel() for p in net.parameters()),
                        bf16=bf16_deviation(ESCRealM, cfg, dict(sd), x, y))
            if cfg["upsampler"] == "dysample":
                p = escrealm_ref.dys_prefix(sd)
                dsd = {"to_img" + k[len(p):]: v for k, v in esc_ref.d64(sd).items() if k.startswith(p + ".")}
                t = got["feat"].double()
                if cfg["mid_dim"] != cfg["dim"]:
                    t = escreal_ref.lrelu(torch.nn.functional.conv2d(t, sd["to_img.0.weight"].double(), sd["to_img.0.bias"].double(), padding=1), 0.01)
                pxs, pys = escreal_ref.dys_positions(t, dsd, S)
                clamped = dict(left=int((pxs < 0).sum()), right=int((pxs > W - 1).sum()), top=int((pys < 0).sum()), bottom=int((pys > H - 1).sum()))
                assert all(v > 0 for v in clamped.values()), clamped
                case["clamped"] = clamped
            np.savez_compressed(f"{HERE}/escrealm_{name}.npz", x=x.numpy(), y=y.numpy(), **arrays)
            meta["cases"][name] = case
    torch.tensor = real_tensor
    with open(f"{HERE}/escrealm_surface.json", "w") as fh:
        json.dump(meta, fh)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))
    for name in escrealm_ref.CASES:
        print(name, os.path.getsize(f"{HERE}/escrealm_{name}.npz"))


if __name__ == "__main__":
    main()
