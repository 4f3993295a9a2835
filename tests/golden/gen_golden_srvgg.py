#!/usr/bin/env python3
"""Golden vectors for SRVGGNetCompact, made by running THE REFERENCE ITSELF (`hat.archs.srvgg_arch.SRVGGNetCompact`, imported with
gen_golden.py's loader shim; build container only).  Data only: weights are regenerated from the seed (tests/srvgg_ref.py's
srvgg_state_dict, conditioned on the case's frame so that every activation map keeps a standard deviation near 1) and never stored.
Writes NEW files only.

  srvgg_a   prelu, 16 convs, x4, 33x40: ragged tiles on both axes       srvgg_b   leakyrelu, 3 convs, x2, 19x35, B = 2
  srvgg_c   relu, 2 convs, x3, 17x18: 27 channels padded to 28          srvgg_d   prelu, 32 convs, x4, 16x16: exactly one tile
  srvgg_e   prelu, 0 convs, x1, 5x3: the degenerate network
Each file: x, y, res = y - nearest(x); a also the map behind layer 8 at srvgg_ref.tap_pixels.  srvgg_surface.json: keys and shapes of the
cases and of the two published configurations (16 and 32 convs, x4, prelu), and per case the reference's own bf16 deviation OF THE
RESIDUAL (net.bfloat16() on the bf16 input against its fp32 output, both with their base image subtracted: PSNR at peak 1 and max-abs;
null where it is not finite).

Asserted per case: std(res) >= 0.1; the negative fraction of every pre-activation in [0.2, 0.8]; the fp64 restatement within 1e-5; for
prelu, distinct slopes per layer, and the output moves by more than 1e-2 max-abs when the slopes are replaced by their channel mean.

    python tests/golden/gen_golden_srvgg.py
"""
from __future__ import annotations

import importlib
import json
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
import srvgg_ref as R  # noqa: E402


def surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def main():
    torch.set_num_threads(4)
    import_reference()
    importlib.import_module("hat.archs.srvgg_arch")
    Net = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("SRVGGNetCompact")
    meta = {"w_seed": R.W_SEED, "x_seed": R.X_SEED, "cases": {}, "surfaces": {}}
    with torch.no_grad():
        for name, cfg in R.SURFACE_CFGS.items():
            net = Net(**cfg)
            assert surface(net) == R.surface_of(cfg)
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net), nparams=sum(p.numel() for p in net.parameters()))
        for name, (cfg, frame) in R.CASES.items():
            net = Net(**cfg).eval()
            assert surface(net) == R.surface_of(cfg), name
            x = R.case_input(name)
            sd = R.srvgg_state_dict(cfg, x)
            net.load_state_dict(sd, strict=True)
            s, n = cfg["upscale"], cfg["num_conv"]
            got = {}
            hooks = []
            if name == R.TAP_CASE:
                hooks.append(net.body[2 * R.TAP_LAYER + 1].register_forward_hook(lambda m, i, o: got.__setitem__("tap", o.clone())))
            y = net(x)
            for h in hooks:
                h.remove()
            assert torch.isfinite(y).all()
            res = y - R.nearest(x, s)
            pre = []
            y64 = R.forward(R.d64(sd), cfg, x.double(), pre=pre)
            err = float((y64 - y.double()).abs().max())
            assert err <= 1e-5, (name, err)
            neg = [float((v < 0).double().mean()) for v in pre]
            assert all(0.2 <= f <= 0.8 for f in neg), (name, neg)
            assert float(res.std()) >= 0.1, (name, float(res.std()))
            case = dict(cfg=cfg, frame=list(frame), out=list(y.shape), surface=surface(net), nparams=sum(p.numel() for p in net.parameters()),
                        res_std=float(res.std()), neg_fraction=[min(neg), max(neg)], fp64_err=err)
            if cfg["act_type"] == "prelu":
                flat = dict(sd)
                for i in range(n + 1):
                    k = f"body.{2 * i + 1}.weight"
                    assert len(set(sd[k].tolist())) == 64, (name, k)
                    flat[k] = torch.full_like(sd[k], float(sd[k].mean()))
                moved = float((R.forward(R.d64(flat), cfg, x.double()) - y64).abs().max())
                assert moved > 1e-2, (name, moved)
                case["mean_slope_moves"] = moved
            netb = Net(**cfg).eval()
            netb.load_state_dict(sd, strict=True)
            xb = x.bfloat16()
            resb = netb.bfloat16()(xb).float() - R.nearest(xb.float(), s)
            p, m = psnr(resb, res), float((resb - res).abs().max())
            case["bf16"] = dict(psnr=p, max_abs=m) if math.isfinite(p) and math.isfinite(m) else None
            arrays = {}
            if name == R.TAP_CASE:
                px = R.tap_pixels(frame[2], frame[3])
                arrays = dict(tap_pixels=px, tap=R.rows_at(got["tap"], px).numpy())
            np.savez_compressed(f"{HERE}/srvgg_{name}.npz", x=x.numpy(), y=y.numpy(), res=res.numpy(), **arrays)
            meta["cases"][name] = case
    with open(f"{HERE}/srvgg_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))
    for name in R.CASES:
        print(name, os.path.getsize(f"{HERE}/srvgg_{name}.npz"))


if __name__ == "__main__":
    main()
