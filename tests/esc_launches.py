"""The cases of tests/golden/esc_launches.json and the one function that runs a case: shared by the generator
(tests/golden/gen_golden_esc_launches.py, run at the commit whose launches are to be pinned) and tests/test_gpu_esc_launches.py.
Public API only (registry.build_network, synth, ops.profile, the networks' and the LTE engine's documented calls), so it runs
against any tree of this project.

Every body is n_blocks=2, conv_blocks=2: the three stream buffers go round, and the second block starts from another buffer than
the first.  Where a whole-model golden (tests/golden/esc*_?.npz) has the configuration, its keywords are taken."""
from __future__ import annotations

import esc_ref
import escfp_ref
import esclte_ref
import escreal_ref
import escrealm_ref

DTYPES = ("bf16", "fp32")
W_SEED, X_SEED = 1234, 4321


def _two(kw, **more):
    return dict(kw, n_blocks=2, conv_blocks=2, **more)


_RM = _two(escrealm_ref.CASES["a"][0])   # ESCRealM x2 behind the /2 unshuffle, nearest+conv: the head runs at x4
CASES = {   # name -> (type, constructor keywords, frame)
    # ESC: use_ln off / on, exp_ratio 1.25 / 2, x2 / x4; 40x72 and 33x64 pad to the 32-pixel windows
    "esc_a": ("ESC", _two(esc_ref.CASES["a"][0]), esc_ref.CASES["a"][1]),
    "esc_b": ("ESC", _two(esc_ref.CASES["b"][0]), esc_ref.CASES["b"][1]),
    # ESCReal, default head: the 64 -> 3 conv runs at width 4 W: 288 (the row-sweep kernel where it is built) and 164 (hat_conv)
    "escreal_w72": ("ESCReal", _two(escreal_ref.CASES["b"][0]), (1, 3, 40, 72)),
    "escreal_w41": ("ESCReal", _two(escreal_ref.CASES["b"][0]), (1, 3, 33, 41)),
    "escreal_dys4": ("ESCReal", _two(escreal_ref.CASES["c"][0]), escreal_ref.CASES["c"][1]),
    "escreal_dys3": ("ESCReal", _two(escreal_ref.CASES["d"][0]), escreal_ref.CASES["d"][1]),
    "escreal_dys2": ("ESCReal", _two(escreal_ref.CASES["e"][0]), escreal_ref.CASES["e"][1]),
    # ESCRealM behind the unshuffle (head scale 4: two r=2 steps).  67x81 and 66x83 are no multiples of f: the corner crop is live.
    # nearest+conv ends in planes at width 4 * 41 = 164 (hat_conv) and 4 * 32 = 128 (a multiple of 16)
    "escrealm_nc_u": ("ESCRealM", _RM, (1, 3, 67, 81)),
    "escrealm_nc_u_w128": ("ESCRealM", _RM, (1, 3, 64, 64)),
    "escrealm_direct_u": ("ESCRealM", _two(escrealm_ref.CASES["b"][0]), escrealm_ref.CASES["b"][1]),   # x1: f = 4
    "escrealm_ps_u": ("ESCRealM", dict(_RM, upsampler="pixelshuffle", mid_dim=64), (1, 3, 64, 64)),      # planes at width 128, 64 channels
    "escrealm_dys48_u": ("ESCRealM", _two(escrealm_ref.CASES["f"][0]), escrealm_ref.CASES["f"][1]),     # `pre` conv present
    "escrealm_dys64_u": ("ESCRealM", dict(_RM, upsampler="dysample", mid_dim=64), (1, 3, 67, 81)),      # `pre` conv absent
    # ESCRealM with the plain stem: head scale 3 (one r=3 step), 4 (two r=2 steps), 2, 1
    "escrealm_nc_x3": ("ESCRealM", _two(escrealm_ref.CASES["c"][0]), escrealm_ref.CASES["c"][1]),       # planes at width 120
    "escrealm_nc_x4": ("ESCRealM", dict(_RM, upscaling_factor=4, unshuffle_mod=False), (1, 3, 33, 40)),  # planes at width 160
    "escrealm_ps_x3": ("ESCRealM", _two(escrealm_ref.CASES["d"][0]), escrealm_ref.CASES["d"][1]),
    "escrealm_ps_x4": ("ESCRealM", _two(escrealm_ref.CASES["e"][0]), escrealm_ref.CASES["e"][1]),
    "escrealm_direct_x2": ("ESCRealM", dict(_RM, upsampler="pixelshuffledirect", unshuffle_mod=False), (1, 3, 33, 40)),
    "escrealm_dys48_x2": ("ESCRealM", dict(_RM, upsampler="dysample", mid_dim=48, unshuffle_mod=False), (1, 3, 33, 40)),
    "escrealm_dys64_x3": ("ESCRealM", dict(_RM, upsampler="dysample", mid_dim=64, upscaling_factor=3), (1, 3, 33, 40)),
    "escrealm_conv_w40": ("ESCRealM", _two(escrealm_ref.CASES["g"][0]), escrealm_ref.CASES["g"][1]),    # upscaling_factor 1: planes at width 40
    "escrealm_conv_w48": ("ESCRealM", _two(escrealm_ref.CASES["g"][0]), (1, 3, 33, 48)),
    "escrealm_conv_x4": ("ESCRealM", dict(_RM, upsampler="conv", upscaling_factor=4), (1, 3, 33, 40)),   # upsampler "conv" at scale 4: no upsampling
    # ESCFP: batches of two
    "escfp_x2": ("ESCFP", _two(escfp_ref.CASES["a"][0]), (2, 3, 40, 72)),
    "escfp_x3": ("ESCFP", _two(escfp_ref.CASES["c"][0]), escfp_ref.CASES["c"][1]),
    "escfp_x4": ("ESCFP", _two(escfp_ref.CASES["b"][0]), (2, 3, 33, 64)),
    # ESC-LTE: gen_feat, query_grid, query, query_grid_u8, query_grid_yuv
    "esclte": ("ESCLTE", _two(esclte_ref.CASES["a"][0]), esclte_ref.CASES["a"][1]),
}
LTE_GRID, LTE_SCATTER = (30, 42), 143   # (an even width: the 4:2:0 frame of the YCbCr sink)


def run_case(name: str, dtype: str, dev, use_graph: bool = False):
    """Build the case's network with seeded weights and run its forward once under ops.profile().
    -> (the (kernel name, tag) pairs in launch order, the outputs as host tensors, the network)."""
    import torch
    from super_resolution_amd import ops, synth, yuv
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    typ, kw, frame = CASES[name]
    net = build_network(dict(kw, type=typ, compute_dtype=dtype, use_graph=use_graph)).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    net = net.to(dev)
    x = synth.synth_input(X_SEED, frame).to(dev)
    outs = []
    with torch.no_grad(), ops.profile() as rec:
        if typ != "ESCLTE":
            outs.append(net(x))
        else:
            h, w = LTE_GRID
            cell = (2.0 / h, 2.0 / w)
            outs.append(net.gen_feat(x * 2 - 1))
            eng = net.engine(dev)
            outs.append(eng.query_grid(h, w, cell))
            coord = synth.uniform(X_SEED, "coord", (LTE_SCATTER, 2)).to(dev) * 2 - 1
            outs.append(eng.query(coord, torch.tensor(cell, device=dev).expand(LTE_SCATTER, 2).contiguous()))
            outs.append(eng.query_grid_u8(torch.zeros(1, h, w, 3, dtype=torch.uint8, device=dev), cell))
            i420 = torch.zeros((1,) + yuv.frame_shape_fmt(h, w, "i420"), dtype=torch.uint8, device=dev)
            eng.query_grid_yuv(ops.yuv_views(i420, "i420"), cell, yuv.csc("bt601", False, 8)[1], (1, 1))
            outs.append(i420)
        torch.cuda.synchronize()
        launches = [[r[0], r[4]] for r in rec]
    return launches, [o.cpu() for o in outs], net
