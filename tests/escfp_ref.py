"""An fp64 restatement of the ESCFP network (esc_fp_arch.py:89-355, eval mode) from its state dict, built on esc_ref's stages: the
goldens under tests/golden/escfp_*.npz come from the reference itself (gen_golden_escfp.py).  Plain torch on the CPU."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import esc_ref as R

GOLDEN, W_SEED, X_SEED, LN_EPS, TAPS = R.GOLDEN, R.W_SEED, R.X_SEED, R.LN_EPS, R.TAPS
BASE = dict(dim=48, pdim=16, kernel_size=13, window_size=32, num_heads=3)
CASES = {   # the whole-model goldens: constructor keywords, frame
    "a": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=1.25, upscaling_factor=2), (1, 3, 40, 72)),   # pads 24 / 24; hidden 72 and 60
    "b": (dict(BASE, n_blocks=2, conv_blocks=2, exp_ratio=2, upscaling_factor=4), (1, 3, 33, 64)),      # pad 31 / 0; hidden 96
    "c": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=1.25, upscaling_factor=3), (2, 3, 33, 40)),   # a batch of two images; odd phase
}
CASE_D = (dict(CASES["a"][0], upscaling_factor=4), (1, 3, 33, 40))   # a's x2 checkpoint in a x4 model: the to_img conversion
SURFACE_CFGS = {f"ESC_FP_X{s}": dict(BASE, n_blocks=5, conv_blocks=5, exp_ratio=1.25, upscaling_factor=s) for s in (2, 3, 4)}

escfp_state_dict = R.esc_state_dict   # every parameter randomised: lk_channel, lk_spatial and plk.proj.3 by synth's fan-in rule
template_from_surface, tap_pixels, d64 = R.template_from_surface, R.tap_pixels, R.d64


def dynamic_kernel(z1, sd, p):
    """z1 (B,16,H,W) -> (B,16,13,13): lk_spatial + the instance's 3x3 padded by 5 (esc_fp_arch.py:106-117), per sample."""
    pooled = z1.mean((2, 3), keepdim=True)
    dyn = F.conv2d(R.gelu(F.conv2d(pooled, sd[p + ".plk.proj.1.weight"], sd[p + ".plk.proj.1.bias"])),
                   sd[p + ".plk.proj.3.weight"], sd[p + ".plk.proj.3.bias"]).reshape(-1, 16, 3, 3)
    return F.pad(dyn, (5, 5, 5, 5)) + sd["lk_spatial"].reshape(1, 16, 13, 13)


def plk_two_step(z, sd, p):
    """esc_fp_arch.py:102-120 as written: conv1x1(lk_channel), then the depthwise 13x13 with each sample's own kernel."""
    z1 = z[:, :16]
    k = dynamic_kernel(z1, sd, p)
    t = F.conv2d(z1, sd["lk_channel"])
    y1 = torch.cat([F.conv2d(t[b:b + 1], k[b].reshape(16, 1, 13, 13), padding=6, groups=16) for b in range(z.shape[0])])
    return torch.cat([y1, z[:, 16:]], 1)


def plk_folded(z, sd, p):
    """The same as one dense conv per sample with weff[o][i] = lk_channel[o][i] * K[o] — what the device path computes."""
    z1 = z[:, :16]
    k = dynamic_kernel(z1, sd, p)
    y1 = torch.cat([F.conv2d(z1[b:b + 1], sd["lk_channel"].reshape(16, 16, 1, 1) * k[b].reshape(16, 1, 13, 13), padding=6)
                    for b in range(z.shape[0])])
    return torch.cat([y1, z[:, 16:]], 1)


def bicubic_phase(x, s, table):
    """x (B,C,H,W) upsampled by the integer factor s from the (s, 4) phase table of packing.bicubic_phase_table: output o reads the
    taps o // s + first .. first + 3, first = -2 if 2 (o % s) + 1 < s else -1, clamped to the frame."""
    def axis(t, dim):
        n = t.shape[dim]
        o = torch.arange(n * s)
        p = o % s
        first = o // s + torch.where(2 * p + 1 < s, -2, -1)
        out = 0
        for a in range(4):
            w = table[p, a].to(t.dtype)
            shape = [1] * t.dim()
            shape[dim] = -1
            out = out + t.index_select(dim, (first + a).clamp(0, n - 1)) * w.reshape(shape)
        return out
    return axis(axis(x, 2), 3)


def forward(sd, cfg, x, taps=None, plk=plk_two_step):
    """The eval forward of ESCFP in the dtype of sd / x (pass d64(sd), x.double() for the fp64 restatement); any batch size."""
    ws, heads, s = cfg["window_size"], cfg["num_heads"], cfg["upscaling_factor"]
    ln = lambda t, k: R.layernorm(t, sd[k + ".weight"], sd[k + ".bias"])
    feat = F.conv2d(x, sd["proj.weight"], sd["proj.bias"], padding=1)
    feat0 = feat
    for i in range(cfg["n_blocks"]):
        p, skip = f"blocks.{i}", feat
        t = R.convffn(ln(feat, p + ".ln_proj"), sd, p + ".proj")
        if taps is not None and i == 0:
            taps["ffn0"] = t
        t = t + R.window_attention(ln(t, p + ".ln_attn"), sd, p + ".attn", ws, heads)
        if taps is not None and i == 0:
            taps["attn0"] = t
        for j in range(cfg["conv_blocks"]):
            z = plk(R.convffn(ln(t, f"{p}.lns.{j}"), sd, f"{p}.convffns.{j}"), sd, f"{p}.pconvs.{j}")
            t = t + F.conv2d(z, sd[f"{p}.pconvs.{j}.aggr.weight"], sd[f"{p}.pconvs.{j}.aggr.bias"])
            if taps is not None and i == 0 and j == 0:
                taps["conv0"] = t
        feat = F.conv2d(ln(t, p + ".ln_out"), sd[p + ".conv_out.weight"], sd[p + ".conv_out.bias"], padding=1) + skip
    feat = F.conv2d(ln(feat, "ln_last"), sd["last.weight"], sd["last.bias"], padding=1) + feat0
    y = F.conv2d(feat, sd["to_img.weight"], sd["to_img.bias"], padding=1)
    return F.pixel_shuffle(y, s) + F.interpolate(x, scale_factor=s, mode="bicubic")


def surfaces() -> dict:
    with open(os.path.join(GOLDEN, "escfp_surface.json")) as f:
        return json.load(f)


def load_case(name: str):
    """-> (cfg, state dict regenerated from the seed, golden arrays, meta) of whole-model case a / b / c / d."""
    meta = surfaces()
    g = dict(np.load(os.path.join(GOLDEN, f"escfp_{name}.npz")))
    cfg = meta["cases"][name]["cfg"]
    sd = escfp_state_dict(template_from_surface(meta["cases"][name]["surface"]), W_SEED)
    return cfg, sd, g, meta["cases"][name]
