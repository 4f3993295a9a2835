"""An fp64 restatement of ESCReal (esc_real_arch.py:312-475, eval mode) from its state dict, built on esc_ref's functions, for the
tests of the device path: `oracle/` is frozen, and the goldens under tests/golden/escreal_*.npz come from the reference itself
(gen_golden_escreal.py).  Plain torch on the CPU; DySample is restated by explicit indexing, not by grid_sample.
dysample_from_rows restates hat_dysample on the kernel's own rows and runs on the rows' device (the multi-trip test's frame)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import esc_ref
from esc_ref import BASE, GOLDEN, W_SEED, X_SEED, d64, tap_pixels, template_from_surface  # noqa: F401
from super_resolution_amd import synth

CASES = {   # the whole-model goldens: constructor keywords, frame
    "a": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=2, upscaling_factor=4), (1, 3, 33, 40)),
    "b": (dict(BASE, n_blocks=2, conv_blocks=2, exp_ratio=1.25, upscaling_factor=2), (1, 3, 40, 72)),   # default head: x4 all the same
    "c": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=2, upscaling_factor=4, use_dysample=True), (1, 3, 33, 40)),
    "d": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=2, upscaling_factor=3, use_dysample=True), (1, 3, 33, 40)),
    "e": (dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=2, upscaling_factor=2, use_dysample=True), (1, 3, 40, 72)),
}
TAP_CASES = ("a", "c", "d", "e")   # the goldens that also keep skip(x) and to_img's input at esc_ref.tap_pixels
FULL = dict(BASE, n_blocks=10, conv_blocks=5, exp_ratio=2, upscaling_factor=4)   # ESC/options/test/ESC_Real_X4.yaml
SURFACE_CFGS = {"ESC_Real_X4": FULL, "ESC_Real_X4_dysample": dict(FULL, use_dysample=True)}
DYS_STD = 0.3   # std of to_img.offset.weight / to_img.scope.weight: positions move by more than two pixels and reach the border clamp


def escreal_state_dict(template: dict, seed: int = W_SEED) -> dict:
    """esc_ref.esc_state_dict for everything (skip.* and the heads fall under synth's name rules), then DySample's offset and
    scope weights at std DYS_STD (the reference's init has scope = 0, which would test nothing) and init_pos as the reference
    computes it (a buffer, not a weight)."""
    sd = esc_ref.esc_state_dict(template, seed)
    for k, v in template.items():
        if k in ("to_img.offset.weight", "to_img.scope.weight"):
            sd[k] = synth.normal(seed, k, tuple(v.shape), std=DYS_STD)
        elif k == "to_img.init_pos":
            sd[k] = init_pos(int(round((v.numel() / 8) ** 0.5))).to(torch.float32)
    return sd


def init_pos(s: int, groups: int = 4) -> torch.Tensor:
    """esc_real_arch.py:352-359 written out: entry d * 4 s^2 + grp * s^2 + i * s + j = h[j] for d = 0 (x), h[i] for d = 1 (y),
    h = (arange(s) - (s - 1) / 2) / s."""
    h = (torch.arange(s, dtype=torch.float64) - (s - 1) / 2) / s
    p = torch.zeros(2, groups, s, s, dtype=torch.float64)
    p[0] = h[None, None, :]
    p[1] = h[None, :, None]
    return p.reshape(1, -1, 1, 1)


def lrelu(x, slope=0.2):
    return torch.where(x >= 0, x, slope * x)


def skip_branch(x, sd):
    """esc_real_arch.py:460-465."""
    h = F.conv2d(x, sd["skip.0.weight"], sd["skip.0.bias"])
    h = F.conv2d(F.pad(h, (3, 3, 3, 3), mode="reflect"), sd["skip.1.weight"], sd["skip.1.bias"], groups=h.shape[1])
    return F.conv2d(lrelu(h), sd["skip.3.weight"], sd["skip.3.bias"])


def nearest2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def head_default(feat, sd):
    """esc_real_arch.py:448-458: two nearest x2 steps, whatever upscaling_factor."""
    t = lrelu(F.conv2d(nearest2(feat), sd["to_img.1.weight"], sd["to_img.1.bias"], padding=1))
    t = lrelu(F.conv2d(nearest2(t), sd["to_img.4.weight"], sd["to_img.4.bias"], padding=1))
    t = lrelu(F.conv2d(t, sd["to_img.6.weight"], sd["to_img.6.bias"], padding=1))
    return F.conv2d(t, sd["to_img.8.weight"], sd["to_img.8.bias"], padding=1)


def dys_positions(feat, sd, s, offset_scale=1.0, groups=4):
    """-> (px, py) (groups, sH, sW): the UNCLAMPED sampling positions in LR pixel units.  The reference's grid value
    2 (c + 0.5 + off) / size - 1, un-normalised with align_corners=False, is c + off exactly."""
    _, _, H, W = feat.shape
    off = F.conv2d(feat, sd["to_img.offset.weight"], sd["to_img.offset.bias"]) * offset_scale
    off = off * torch.sigmoid(F.conv2d(feat, sd["to_img.scope.weight"])) * 0.5 + sd["to_img.init_pos"].to(feat.dtype)
    # channel d * 4 s^2 + grp * s^2 + i * s + j -> axis d of group grp at output pixel (s y + i, s x + j)
    off = off.reshape(2, groups, s, s, H, W).permute(0, 1, 4, 2, 5, 3).reshape(2, groups, s * H, s * W)
    xs = torch.arange(s * W, dtype=feat.dtype).div(s, rounding_mode="floor")[None, None, :]
    ys = torch.arange(s * H, dtype=feat.dtype).div(s, rounding_mode="floor")[None, :, None]
    return xs + off[0], ys + off[1]


def bilinear_border(m, px, py):
    """m (C, H, W) sampled at positions (px, py) (sH, sW) clamped to the frame -> (C, sH, sW)."""
    _, H, W = m.shape
    px, py = px.clamp(0, W - 1), py.clamp(0, H - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    tx, ty = px - x0, py - y0
    return (m[:, y0, x0] * (1 - tx) * (1 - ty) + m[:, y0, x1] * tx * (1 - ty) + m[:, y1, x0] * (1 - tx) * ty + m[:, y1, x1] * tx * ty)


def head_dysample(feat, sd, s, offset_scale=1.0, project_first=False, groups=4):
    """esc_real_arch.py:361-399.  project_first: end_conv per group in front of the sampling (what hat_dysample reads)."""
    px, py = dys_positions(feat, sd, s, offset_scale, groups)
    cg = feat.shape[1] // groups
    we, be = sd["to_img.end_conv.weight"].reshape(3, -1), sd["to_img.end_conv.bias"]
    if project_first:
        y = be[:, None, None].expand(3, px.shape[1], px.shape[2]).clone()
        for g in range(groups):
            proj = torch.einsum("oc,chw->ohw", we[:, cg * g: cg * (g + 1)], feat[0, cg * g: cg * (g + 1)])
            y = y + bilinear_border(proj, px[g], py[g])
        return y[None]
    up = torch.cat([bilinear_border(feat[0, cg * g: cg * (g + 1)], px[g], py[g]) for g in range(groups)], 0)
    return F.conv2d(up[None], sd["to_img.end_conv.weight"], be)


def dysample_from_rows(rows, init_pos, bias, H, W, s, band=None, groups=4):
    """hat_dysample restated in fp64 on the kernel's own operands, on the rows' device.  rows (B, H*W, ld) = [offset 8 s^2 | scope
    8 s^2 | groups x 3 projected values | pad], entry d * 4 s^2 + grp * s^2 + i * s + j of offset / scope / init_pos being axis d
    (0: x, 1: y) of group grp at output pixel (s y + i, s x + j); init_pos (8 s^2,); bias (3,) -> (B, 3, sH, sW) fp64.
    `band`: LR rows handled at a time (None: all); only a band's positions and gathers exist next to the result."""
    B, ss, dev = rows.shape[0], s * s, rows.device
    m = rows.reshape(B, H, W, rows.shape[-1])
    proj = m[..., 16 * ss: 16 * ss + 3 * groups].double().reshape(B, H * W, groups, 3)
    ip = init_pos.double().reshape(2, groups, s, s).to(dev)
    out = torch.empty(B, 3, s * H, s * W, dtype=torch.float64, device=dev)
    xs = torch.arange(W, dtype=torch.float64, device=dev)[None, None, :, None, None, None]
    band = H if band is None else band
    for r0 in range(0, H, band):
        r1 = min(r0 + band, H)
        n = r1 - r0
        blk = m[:, r0:r1, :, :16 * ss].double()
        off = blk[..., :8 * ss].reshape(B, n, W, 2, groups, s, s)
        scope = blk[..., 8 * ss:].reshape(B, n, W, 2, groups, s, s)
        pos = off * torch.sigmoid(scope) * 0.5 + ip
        ys = torch.arange(r0, r1, dtype=torch.float64, device=dev)[None, :, None, None, None, None]
        px, py = (pos[:, :, :, 0] + xs).clamp(0, W - 1), (pos[:, :, :, 1] + ys).clamp(0, H - 1)     # (B, n, W, groups, s, s)
        x0, y0 = px.floor().long(), py.floor().long()
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
        tx, ty = px - x0, py - y0
        acc = bias.double().to(dev).reshape(1, 1, 1, 1, 1, 3).expand(B, n, W, s, s, 3).clone()
        for g in range(groups):
            pg = proj[:, :, g]
            take = lambda yy, xx: torch.gather(pg, 1, (yy[:, :, :, g] * W + xx[:, :, :, g]).reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, n, W, s, s, 3)
            wx, wy = tx[:, :, :, g, :, :, None], ty[:, :, :, g, :, :, None]
            acc += take(y0, x0) * (1 - wx) * (1 - wy) + take(y0, x1) * wx * (1 - wy) + take(y1, x0) * (1 - wx) * wy + take(y1, x1) * wx * wy
        out[:, :, s * r0: s * r1] = acc.permute(0, 5, 1, 3, 2, 4).reshape(B, 3, n * s, W * s)
    return out


def trunk(sd, cfg, x):
    """proj and the blocks of ESC with use_ln (esc_ref.forward's loop) -> (feat0, the stream after the last block)."""
    ws, heads, pdim = cfg["window_size"], cfg["num_heads"], cfg["pdim"]
    lk = esc_ref.geo_ensemble(sd["plk_filter"])
    feat = feat0 = F.conv2d(x, sd["proj.weight"], sd["proj.bias"], padding=1)
    for i in range(cfg["n_blocks"]):
        p, skip = f"blocks.{i}", feat
        t = esc_ref.convffn(esc_ref.layernorm(feat, sd[p + ".ln_proj.weight"], sd[p + ".ln_proj.bias"]), sd, p + ".proj")
        t = t + esc_ref.window_attention(esc_ref.layernorm(t, sd[p + ".ln_attn.weight"], sd[p + ".ln_attn.bias"]), sd, p + ".attn", ws, heads)
        for j in range(cfg["conv_blocks"]):
            n = esc_ref.layernorm(t, sd[f"{p}.lns.{j}.weight"], sd[f"{p}.lns.{j}.bias"])
            z = esc_ref.plk(esc_ref.convffn(n, sd, f"{p}.convffns.{j}"), sd, f"{p}.pconvs.{j}", lk, pdim)
            t = t + F.conv2d(z, sd[f"{p}.pconvs.{j}.aggr.weight"], sd[f"{p}.pconvs.{j}.aggr.bias"])
        feat = F.conv2d(esc_ref.layernorm(t, sd[p + ".ln_out.weight"], sd[p + ".ln_out.bias"]), sd[p + ".conv_out.weight"],
                        sd[p + ".conv_out.bias"], padding=1) + skip
    return feat0, feat


def forward(sd, cfg, x, taps=None):
    """The eval forward of ESCReal in the dtype of sd / x.  taps receives skip(x) and to_img's input."""
    if x.shape[0] != 1:
        raise RuntimeError("ESCReal's eval path takes one frame at a time")
    feat0, feat = trunk(sd, cfg, x)
    sk = skip_branch(x, sd)
    feat = F.conv2d(feat, sd["last.weight"], sd["last.bias"], padding=1) + feat0 + sk
    if taps is not None:
        taps["skip"], taps["feat"] = sk, feat
    if cfg.get("use_dysample", False):
        return head_dysample(feat, sd, cfg["upscaling_factor"])
    return head_default(feat, sd)


def rows_at(t, px):
    """(1, C, H, W) -> (len(px), C) at flat pixel indices px."""
    return t[0].reshape(t.shape[1], -1)[:, torch.as_tensor(px)].t().contiguous()


def surfaces() -> dict:
    with open(os.path.join(GOLDEN, "escreal_surface.json")) as f:
        return json.load(f)


def load_case(name: str):
    """-> (cfg, state dict regenerated from the seed, golden arrays, meta) of whole-model case a .. e."""
    meta = surfaces()
    g = dict(np.load(os.path.join(GOLDEN, f"escreal_{name}.npz")))
    cfg = meta["cases"][name]["cfg"]
    sd = escreal_state_dict(template_from_surface(meta["cases"][name]["surface"]), W_SEED)
    return cfg, sd, g, meta["cases"][name]
