#!/usr/bin/env python3
"""Golden vectors for HybridHATNAF, made like gen_golden_hatx.py by running THE REFERENCE ITSELF
(`hat.archs.hybrid_hat_naf_arch.HybridHATNAF`, imported with the same loader shim; build container only).  Data only; weights
are regenerated from the seed and never stored.  Writes NEW files only: the configs and state-dict surfaces go to
naf_surface.json (meta.json and state_dict_surface.json are not touched).

  whole_hybrid_w64_x2   naf_width 64, 4 blocks in front of gen_golden_hatx.TINY (overlap 0.5, window 8, x2), frame 16x24:
                        y and x_naf (the stem's output: a failure can be placed in the stem or after it)
  whole_hybrid_w32_x2   naf_width 32, 2 blocks, same frame
  blocks_naf            on a 20x37 map (ragged in both axes, odd width), for both widths: one NAFBlock on a seeded (1,c,20,37)
                        input, its attention half alone (y), and the whole NAFStem on a (1,3,20,37) image

    python tests/golden/gen_golden_naf.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from gen_golden import W_SEED, X_SEED, import_reference  # noqa: E402
from gen_golden_hatx import TINY  # noqa: E402
from super_resolution_amd import synth  # noqa: E402

HAT_KW = dict(TINY, overlap_ratio=0.5, window_size=8, upscale=2)
CFGS_NAF = {
    "hybrid_w64_x2": dict(naf_width=64, naf_blocks=4, hat_kwargs=HAT_KW),
    "hybrid_w32_x2": dict(naf_width=32, naf_blocks=2, hat_kwargs=HAT_KW),
}
FRAME, MAP = (1, 3, 16, 24), (20, 37)


def main():
    torch.set_num_threads(4)
    import_reference()
    importlib.import_module("hat.archs.hybrid_hat_naf_arch")
    Hybrid = sys.modules["basicsr.utils.registry"].ARCH_REGISTRY.get("HybridHATNAF")
    out = {"w_seed": W_SEED, "x_seed": X_SEED, "cfgs": CFGS_NAF, "surfaces": {}, "nparams": {}, "attrs": {}}
    blocks = {"hw": np.array(MAP)}
    with torch.no_grad():
        for name, cfg in CFGS_NAF.items():
            net = Hybrid(**cfg).eval()
            out["surfaces"][name] = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
            out["nparams"][name] = sum(p.numel() for p in net.parameters())
            out["attrs"][name] = dict(window_size=net.window_size, upscale=net.upscale, in_chans=net.in_chans, img_range=net.img_range,
                                      extra_repr=net.extra_repr())
            net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
            x = synth.synth_input(X_SEED, FRAME)
            np.savez(f"{HERE}/whole_{name}.npz", y=net(x).numpy(), x_naf=net.naf(x).numpy(), x_shape=np.array(FRAME))
            c = cfg["naf_width"]
            t = synth.normal(X_SEED, f"naf_in_c{c}", (1, c) + MAP)
            blk = net.naf.body[0]
            g = blk.sg(blk.dw(blk.pw1(t)))
            blocks[f"half_c{c}"] = (t + blk.beta * blk.pw2(g * blk.sca(g))).numpy()
            blocks[f"block_c{c}"] = blk(t).numpy()
            blocks[f"stem_c{c}"] = net.naf(synth.synth_input(X_SEED, (1, 3) + MAP)).numpy()
    # the merge rules of hybrid_hat_naf_arch.py:109-118 on constructor arguments the fixtures do not use
    small = dict(TINY, overlap_ratio=0.5)
    for key, kw in {"top_level_wins": dict(window_size=4, hat_kwargs=dict(small, window_size=8)),
                    "hat_kwargs_window": dict(hat_kwargs=dict(small, window_size=4)),
                    "hat_kwargs_upscale_wins": dict(upscale=4, hat_kwargs=dict(small, upscale=2)),
                    "top_level_upscale_fills": dict(upscale=4, naf_blocks=1, naf_width=32,
                                                    hat_kwargs={k: v for k, v in small.items() if k != "upscale"})}.items():
        net = Hybrid(**kw)
        out["attrs"]["merge:" + key] = dict(kwargs=kw, window_size=net.window_size, upscale=net.upscale, in_chans=net.in_chans,
                                            hat_window_size=net.hat.window_size, hat_upscale=net.hat.upscale)
    np.savez(f"{HERE}/blocks_naf.npz", **blocks)
    with open(f"{HERE}/naf_surface.json", "w") as f:
        json.dump(out, f)
    print("HybridHATNAF goldens written")


if __name__ == "__main__":
    main()
