#!/usr/bin/env python3
"""Golden vectors for RRDBNet, made by running THE REFERENCE ITSELF (`basicsr.archs.rrdbnet_arch.RRDBNet`, imported with gen_golden.py's
loader shim plus the reference's own arch_util behind stubs for the packages it imports and this network never calls; build
container only).  Data only: weights are regenerated from the seed (tests/rrdb_ref.py's rrdb_state_dict, conditioned on the case's
frame) and never stored.  Writes NEW files only.

  rrdb_a   2 blocks, x4, 33x40: ragged tiles on both axes        rrdb_b   1 block, x2, 38x34, B = 2: the body at 19x17
  rrdb_c   1 block, x1, 20x36: the body at 5x9                   rrdb_d   23 blocks, x4, 16x16: the published depth on exactly one tile
  rrdb_e   0 blocks, x4, 5x3: the degenerate network
Each file: x, y; a also the stream behind RRDB 0 at rrdb_ref.tap_pixels.  rrdb_surface.json: keys and shapes of the cases and of the
two published configurations (23 blocks, x4 and x2), and per case the reference's own all-bf16 deviation (net.bfloat16() on the bf16
input against its fp32 output: PSNR at peak 1 and max-abs).

Asserted per case: the fp64 restatement within 1e-5; std(y) in [0.1, 1]; the negative fraction of every conv 1-4 pre-activation in
[0.2, 0.8]; with blocks, the output moves by more than 1e-2 max-abs when x4 is zeroed before conv 5 and when 0.2 (slope and residual
scale) is replaced by 0.25 in the restatement; the reference's bf16 PSNR >= 40 dB.

    python tests/golden/gen_golden_rrdb.py
"""
from __future__ import annotations

import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden as G  # noqa: E402
import rrdb_ref as R  # noqa: E402


def import_rrdbnet():
    G.import_reference()

    def stub(name, **kw):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(kw)
            sys.modules[name] = m
        else:
            sys.modules[name].__dict__.update(kw)

    try:
        importlib.import_module("torchvision")
    except ImportError:
        stub("torchvision", __version__="0.0.0")
    stub("basicsr.ops")
    stub("basicsr.ops.dcn", ModulatedDeformConvPack=torch.nn.Module, modulated_deform_conv=None)   # DCNv2Pack's base: never built here
    stub("basicsr.utils", get_root_logger=lambda: None)
    archs = f"{G.REF}/ESC/basicsr/archs"
    for name in ("arch_util", "rrdbnet_arch"):
        spec = importlib.util.spec_from_file_location(f"basicsr.archs.{name}", f"{archs}/{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"basicsr.archs.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("RRDBNet")


def surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def main():
    torch.set_num_threads(4)
    Net = import_rrdbnet()
    meta = {"w_seed": R.W_SEED, "x_seed": R.X_SEED, "cases": {}, "surfaces": {}}
    with torch.no_grad():
        for name, cfg in R.SURFACE_CFGS.items():
            net = Net(**cfg)
            assert surface(net) == R.surface_of(cfg)
            meta["surfaces"][name] = dict(cfg=cfg, surface=surface(net), nparams=sum(p.numel() for p in net.parameters()))
        for name, (cfg, frame, gain) in R.CASES.items():
            net = Net(**cfg).eval()
            assert surface(net) == R.surface_of(cfg), name
            x = R.case_input(name)
            sd = R.rrdb_state_dict(cfg, x, gain)
            net.load_state_dict(sd, strict=True)
            got = {}
            hooks = []
            if name == R.TAP_CASE:
                hooks.append(net.body[R.TAP_BLOCK].register_forward_hook(lambda m, i, o: got.__setitem__("tap", o.clone())))
            y = net(x)
            for h in hooks:
                h.remove()
            assert torch.isfinite(y).all()
            pre = []
            sd64 = R.d64(sd)
            y64 = R.forward(sd64, cfg, x.double(), pre=pre)
            err = float((y64 - y.double()).abs().max())
            assert err <= 1e-5, (name, err)
            assert 0.1 <= float(y.std()) <= 1.0, (name, float(y.std()))
            case = dict(cfg=cfg, frame=list(frame), out=list(y.shape), gain=gain, surface=surface(net), nparams=sum(p.numel() for p in net.parameters()),
                        y_std=float(y.std()), fp64_err=err)
            if cfg["num_block"]:
                neg = [float((v < 0).double().mean()) for v in pre]
                assert all(0.2 <= f <= 0.8 for f in neg), (name, min(neg), max(neg))
                no_x4 = float((R.forward(sd64, cfg, x.double(), drop_x4=True) - y64).abs().max())
                other = float((R.forward(sd64, cfg, x.double(), slope=0.25, beta=0.25) - y64).abs().max())
                assert no_x4 > 1e-2 and other > 1e-2, (name, no_x4, other)
                case.update(neg_fraction=[min(neg), max(neg)], zeroed_x4_moves=no_x4, quarter_moves=other)
            netb = Net(**cfg).eval()
            netb.load_state_dict(sd, strict=True)
            yb = netb.bfloat16()(x.bfloat16()).float()
            case["bf16"] = dict(psnr=psnr(yb, y), max_abs=float((yb - y).abs().max()))
            assert case["bf16"]["psnr"] >= 40.0, (name, case["bf16"])
            arrays = {}
            if name == R.TAP_CASE:
                px = R.tap_pixels(frame[2], frame[3])
                arrays = dict(tap_pixels=px, tap=R.rows_at(got["tap"], px).numpy())
            np.savez_compressed(f"{HERE}/rrdb_{name}.npz", x=x.numpy(), y=y.numpy(), **arrays)
            meta["cases"][name] = case
    with open(f"{HERE}/rrdb_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))
    for name in R.CASES:
        print(name, os.path.getsize(f"{HERE}/rrdb_{name}.npz"))


if __name__ == "__main__":
    main()
