#!/usr/bin/env python3
"""Golden vectors for ESC-LTE, made by running THE REFERENCE ITSELF: ESC/esc_arb's `models.lte.LTE` over `models.esc.Net` with
`models.mlp.MLP`, built through the reference's own classes and registry (build container only).  Shims, none of which touches the
forward arithmetic: the `models` package is entered without its __init__ (which imports every baseline model), `utils` is loaded by
path with an empty `tensorboardX`, `Tensor.cuda()` is the identity (lte.py:25 calls it on the feature coordinates), and an encoder
name `esc-small` is registered that passes its arguments on to `Net` (the reference's own `esc` ignores them and always builds 5 x 5
blocks).  Data only: weights are regenerated from the seed (tests/esclte_ref.py's lte_state_dict) and never stored.

  esclte_a   a 20x24 frame on the make_coord grid of 30x41 (x1.5 / x1.708: unequal axes)
  esclte_b   the same frame at x1: every rel is 0 or +-2, the 1e-9 area term decides
  esclte_c   x5 with scale_max 4: the cell is clipped
  esclte_d   143 scattered coordinates with exactly -1 and 1 on both axes (the clamp); n_blocks 2
Each file: x (the normalised input), coord, cell, y.  esclte_surface.json: keys and shapes of the cases and of the model of
train_esc-lte.yaml, the seeds, the factor on the last imnet layer, and per case the output's range.

    python tests/golden/gen_golden_esclte.py
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

from gen_golden import REF  # noqa: E402
import esclte_ref as R  # noqa: E402
from super_resolution_amd import synth  # noqa: E402

ARB = REF + "/ESC/esc_arb"


def import_reference_lte():
    sys.dont_write_bytecode = True
    sys.modules["tensorboardX"] = types.SimpleNamespace(SummaryWriter=object)
    spec = importlib.util.spec_from_file_location("utils", ARB + "/utils.py")
    utils = importlib.util.module_from_spec(spec)
    sys.modules["utils"] = utils
    spec.loader.exec_module(utils)
    pkg = types.ModuleType("models")
    pkg.__path__ = [ARB + "/models"]
    sys.modules["models"] = pkg
    core = importlib.import_module("models.models")
    pkg.register, pkg.make = core.register, core.make
    for m in ("mlp", "esc", "lte"):
        importlib.import_module("models." + m)
    Net = sys.modules["models.esc"].Net
    core.register("esc-small")(lambda **kw: Net(**kw))
    torch.Tensor.cuda = lambda self, *a, **k: self
    return core, utils


def surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def build(core, enc_name, enc_args):
    spec = dict(name="lte", args=dict(encoder_spec=dict(name=enc_name, args=enc_args),
                                      imnet_spec=dict(name="mlp", args=dict(out_dim=3, hidden_list=[R.HIDDEN] * 3)), hidden_dim=R.HIDDEN))
    return core.make(spec).eval()


def main():
    torch.set_num_threads(4)
    core, utils = import_reference_lte()
    meta = {"w_seed": R.W_SEED, "x_seed": R.X_SEED, "last_scale": R.LAST_SCALE, "cases": {}, "surfaces": {}}
    with torch.no_grad():
        net = build(core, "esc", dict(no_upsampling=True))
        meta["surfaces"]["ESC_LTE"] = dict(cfg=dict(R.ENC, n_blocks=5, conv_blocks=5), surface=surface(net),
                                           nparams=sum(p.numel() for p in net.parameters()))
        for name, (cfg, frame, what) in R.CASES.items():
            net = build(core, "esc-small", dict(cfg))
            net.load_state_dict(R.lte_state_dict(net.state_dict(), R.W_SEED, R.LAST_SCALE), strict=True)
            x = (synth.synth_input(R.X_SEED, frame) - 0.5) / 0.5
            coord, cell = R.case_queries(name)
            if "grid" in what:   # the coordinates the reference's own make_coord gives
                assert torch.equal(coord, utils.make_coord(what["grid"]))
            y = net(x, coord[None].clone(), cell[None].clone())
            np.savez(f"{HERE}/esclte_{name}.npz", x=x.numpy(), coord=coord.numpy(), cell=cell.numpy(), y=y[0].numpy())
            meta["cases"][name] = dict(cfg=cfg, frame=list(frame), what=what, surface=surface(net),
                                       y_min=float(y.min()), y_max=float(y.max()), y_std=float(y.std()))
    with open(f"{HERE}/esclte_surface.json", "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("surface", "cfg")} for k, v in meta["cases"].items()}, indent=1))


if __name__ == "__main__":
    main()
