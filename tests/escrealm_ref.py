"""An fp64 restatement of ESCRealM (esc_real_arch.py:478-661, eval mode) from its state dict, on top of escreal_ref's functions, for
the tests of the device path: check_img_size + PixelUnshuffle by index, the skip branch over the unshuffled channels, UniUpsample's
five heads, the whole net.  The goldens under tests/golden/escrealm_*.npz come from the reference itself
(gen_golden_escrealm.py).  Plain torch on the CPU."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import esc_ref
import escreal_ref
from esc_ref import BASE, GOLDEN, W_SEED, X_SEED, d64, tap_pixels, template_from_surface  # noqa: F401
from escreal_ref import DYS_STD, init_pos, lrelu, rows_at  # noqa: F401
from super_resolution_amd import synth

UPSAMPLERS = ("conv", "pixelshuffledirect", "pixelshuffle", "nearest+conv", "dysample")   # MetaUpsample's method index
_ONE = dict(BASE, n_blocks=1, conv_blocks=1, exp_ratio=2)
CASES = {   # the whole-model goldens: constructor keywords, frame
    "a": (dict(_ONE, upscaling_factor=2, upsampler="nearest+conv"), (1, 3, 67, 81)),          # unshuffle f=2, body 34x41
    "b": (dict(_ONE, upscaling_factor=1, upsampler="pixelshuffledirect"), (1, 3, 66, 83)),    # unshuffle f=4, pads 2 and 1, body 17x21
    "c": (dict(_ONE, upscaling_factor=3, upsampler="nearest+conv"), (1, 3, 33, 40)),
    "d": (dict(_ONE, upscaling_factor=3, upsampler="pixelshuffle", mid_dim=48), (1, 3, 33, 40)),
    "e": (dict(BASE, n_blocks=2, conv_blocks=2, exp_ratio=1.25, upscaling_factor=4, unshuffle_mod=False, upsampler="pixelshuffle", mid_dim=48),
          (1, 3, 33, 40)),
    "f": (dict(_ONE, upscaling_factor=2, upsampler="dysample", mid_dim=48), (1, 3, 67, 81)),  # unshuffle f=2, DySample x4 on 48 channels
    "g": (dict(_ONE, upscaling_factor=1, unshuffle_mod=False, upsampler="conv"), (1, 3, 33, 40)),
}
TAP_CASES = ("a", "b", "c", "f")   # the goldens that also keep skip(x) and to_img's input at esc_ref.tap_pixels of the body's frame
FULL = dict(BASE, n_blocks=10, conv_blocks=5, exp_ratio=2, upscaling_factor=4)   # ESC_Real_X4's size
SURFACE_CFGS = {f"ESC_Real_X4_{u}": dict(FULL, upsampler=u) for u in UPSAMPLERS}


def stem_of(cfg):
    """-> (unshuffle factor f or 0, the head's scale S)."""
    s = cfg["upscaling_factor"]
    return (4 // s, 4) if cfg.get("unshuffle_mod", True) and s < 3 else (0, s)


def dys_prefix(sd):
    return next(k for k in sd if k.endswith("offset.weight"))[:-len(".offset.weight")]


def meta_upsample(cfg):
    _, S = stem_of(cfg)
    return [2, UPSAMPLERS.index(cfg.get("upsampler", "nearest+conv")), S, cfg["dim"], 3, cfg.get("mid_dim", 48), 4]


def escrealm_state_dict(template: dict, cfg: dict, seed: int = W_SEED) -> dict:
    """esc_ref.esc_state_dict for everything, DySample's offset / scope weights at std DYS_STD and init_pos as the reference
    computes it (escreal_ref.escreal_state_dict's rules under UniUpsample's key prefix), MetaUpsample as the reference fills it."""
    sd = esc_ref.esc_state_dict({k: v for k, v in template.items() if not k.endswith("MetaUpsample")}, seed)
    for k, v in template.items():
        if k.endswith((".offset.weight", ".scope.weight")):
            sd[k] = synth.normal(seed, k, tuple(v.shape), std=DYS_STD)
        elif k.endswith(".init_pos"):
            sd[k] = init_pos(int(round((v.numel() / 8) ** 0.5))).to(torch.float32)
    sd["to_img.MetaUpsample"] = torch.tensor(meta_upsample(cfg), dtype=torch.uint8)
    return sd


def unshuffle_pad(x, f):
    """check_img_size (reflect pad right / bottom to a multiple of f) and PixelUnshuffle(f), by index: channel c f^2 + f i + j of
    (yb, xb) is x[c][refl(f yb + i)][refl(f xb + j)]."""
    B, C, h, w = x.shape
    Hb, Wb = -(-h // f), -(-w // f)
    xp = x[:, :, esc_ref.reflect_index(h, Hb * f)][:, :, :, esc_ref.reflect_index(w, Wb * f)]
    return xp.reshape(B, C, Hb, f, Wb, f).permute(0, 1, 3, 5, 2, 4).reshape(B, C * f * f, Hb, Wb)


def skip_branch(xu, sd, first=0):
    """esc_real_arch.py:613-628 behind the unshuffle (first = 1) or on the frame (first = 0)."""
    k = [f"skip.{first + i}" for i in (0, 1, 3)]
    h = F.conv2d(xu, sd[k[0] + ".weight"], sd[k[0] + ".bias"])
    h = F.conv2d(F.pad(h, (3, 3, 3, 3), mode="reflect"), sd[k[1] + ".weight"], sd[k[1] + ".bias"], groups=h.shape[1])
    return F.conv2d(lrelu(h), sd[k[2] + ".weight"], sd[k[2] + ".bias"])


def nearest(x, r):
    return x.repeat_interleave(r, dim=2).repeat_interleave(r, dim=3)


def pixel_shuffle(x, r):
    B, C, H, W = x.shape
    return x.reshape(B, C // (r * r), r, r, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, C // (r * r), H * r, W * r)


def _conv(t, sd, i):
    return F.conv2d(t, sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], padding=1)


def head(feat, sd, upsampler, S, mid_dim=48):
    """UniUpsample.forward (esc_real_arch.py:478-574) at scale S, by the Sequential's own numbering."""
    if S == 1 or upsampler == "conv":
        return _conv(feat, sd, 0)
    steps = [3] if S == 3 else [2] * (S // 2)
    if upsampler == "pixelshuffledirect":
        return pixel_shuffle(_conv(feat, sd, 0), S)
    if upsampler == "pixelshuffle":
        t, i = lrelu(_conv(feat, sd, 0), 0.01), 2
        for r in steps:
            t, i = pixel_shuffle(_conv(t, sd, i), r), i + 2
        return _conv(t, sd, i)
    if upsampler == "nearest+conv":
        t, i = feat, 0
        for r in steps:   # conv FIRST, then nearest, then the activation
            t, i = lrelu(nearest(_conv(t, sd, i), r)), i + 3
        return _conv(lrelu(_conv(t, sd, i)), sd, i + 2)
    if upsampler == "dysample":
        t = feat
        if mid_dim != feat.shape[1]:
            t = lrelu(_conv(feat, sd, 0), 0.01)
        p = dys_prefix(sd)
        return escreal_ref.head_dysample(t, {"to_img" + k[len(p):]: v for k, v in sd.items() if k.startswith(p + ".")}, S)
    raise ValueError(upsampler)


def forward(sd, cfg, x, taps=None):
    """The eval forward of ESCRealM in the dtype of sd / x.  taps receives skip(x) and to_img's input (at the body's size)."""
    if x.shape[0] != 1:
        raise RuntimeError("ESCRealM's eval path takes one frame at a time")
    f, S = stem_of(cfg)
    s, (h, w) = cfg["upscaling_factor"], x.shape[-2:]
    xu = unshuffle_pad(x, f) if f else x
    body = dict(sd)
    if f:
        body["proj.weight"], body["proj.bias"] = sd["proj.1.weight"], sd["proj.1.bias"]
    feat0, feat = escreal_ref.trunk(body, cfg, xu)
    sk = skip_branch(xu, sd, 1 if f else 0)
    feat = F.conv2d(feat, sd["last.weight"], sd["last.bias"], padding=1) + feat0 + sk
    if taps is not None:
        taps["skip"], taps["feat"] = sk, feat
    y = head(feat, sd, cfg.get("upsampler", "nearest+conv"), S, cfg.get("mid_dim", 48))
    return y[:, :, :h * s, :w * s]


def surfaces() -> dict:
    with open(os.path.join(GOLDEN, "escrealm_surface.json")) as fh:
        return json.load(fh)


def load_case(name: str):
    """-> (cfg, state dict regenerated from the seed, golden arrays, meta) of whole-model case a .. g."""
    meta = surfaces()
    g = dict(np.load(os.path.join(GOLDEN, f"escrealm_{name}.npz")))
    cfg = meta["cases"][name]["cfg"]
    sd = escrealm_state_dict(template_from_surface(meta["cases"][name]["surface"]), cfg, W_SEED)
    return cfg, sd, g, meta["cases"][name]
