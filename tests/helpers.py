"""Shared helpers for the tests: golden loading, oracle nets with synthetic weights, the per-kernel GPU tests' input / tolerance
helpers, and plain fp64 restatements of the HATX attention options and the SGFN gate that take the kernels' own inputs."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hat_oracle as O
from super_resolution_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "meta.json")) as f:
    META = json.load(f)
W_SEED, X_SEED = META["w_seed"], META["x_seed"]


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def cfg_of(name):
    return O.make_cfg(**META["cfgs"][name])


def oracle_sd(name):
    cfg = cfg_of(name)
    return cfg, synth.synth_state_dict(O.blank_state_dict(cfg), W_SEED)


def max_abs(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


WMSA_CASES = ["wmsa_c48_h2_ws16", "wmsa_c48_h6_ws8"]


def wmsa_sd(C, heads, ws):
    """Synthetic WindowAttention parameters: same keys / shapes / seeded generator as gen_golden_wmsa.py (the integer
    relative_position_index is a deterministic function of ws and carries no randomness)."""
    blank = {"relative_position_bias_table": torch.zeros((2 * ws - 1) ** 2, heads),
             "relative_position_index": O.rpi_sa(ws),
             "qkv.weight": torch.zeros(3 * C, C), "qkv.bias": torch.zeros(3 * C),
             "proj.weight": torch.zeros(C, C), "proj.bias": torch.zeros(C)}
    return synth.synth_state_dict(blank, W_SEED)


# ------------------------------------------------------------------------------------------------
# per-kernel GPU tests (test_gpu_ops.py, test_gpu_hatx_ops.py): inputs and the project's tolerance bars
# ------------------------------------------------------------------------------------------------
def _r8(x):
    return (x + 7) // 8 * 8


def to_dev(x_bhwc: torch.Tensor, ld: int, tdt, dev):
    """(B,H,W,C) float -> device (B, H*W, ld) of dtype tdt with zero pad channels."""
    b, h, w, c = x_bhwc.shape
    out = torch.zeros(b, h * w, ld, dtype=tdt, device=dev)
    out[:, :, :c] = x_bhwc.reshape(b, h * w, c).to(dev).to(tdt)
    return out


def check(got: torch.Tensor, ref: torch.Tensor, dtype: str, what: str, f32_tol=2e-5):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    rel = float((got - ref).norm() / max(float(ref.norm()), 1e-12))
    if dtype == "f32":
        assert err <= f32_tol * max(scale, 1.0), f"{what}: max-abs {err:.3e} (scale {scale:.3g}, rel {rel:.3e})"
    else:
        assert rel <= 1.2e-2 and err <= 6e-2 * max(scale, 1.0), f"{what}: rel {rel:.3e} max-abs {err:.3e} (scale {scale:.3g})"


def rnd(key, shape, std=1.0):
    return synth.normal(11, key, shape, std=std)


def q(x, dtype):
    """Round inputs the way the kernel's storage type does, so the oracle sees the same operands."""
    return x.to(torch.bfloat16).to(torch.float32) if dtype == "bf16" else x


# ------------------------------------------------------------------------------------------------
# fp64 restatements of hat_ocab_keybias / hat_ocab_attention_kb / hat_sgfn_gate (include/hat_mi355x.h), written on the kernels'
# own inputs and by index arithmetic (no unfold), so that they share no code with oracle/hat_oracle.py; test_hatx_ops_ref_cpu.py
# pins them to it.
# ------------------------------------------------------------------------------------------------
def key_windows(x: torch.Tensor, ws: int, wse: int, pad: int):
    """(B,H,W,...) -> ((B, nWy, nWx, wse*wse, ...) values of every key window, 0 outside the image; (nWy, nWx, wse*wse) bool:
    the key is a pixel of the image).  Key `kh * wse + kw` of window (wy, wx) is pixel (wy*ws - pad + kh, wx*ws - pad + kw)."""
    b, h, w = x.shape[:3]
    nwy, nwx = h // ws, w // ws
    key = torch.arange(wse * wse)
    y = torch.arange(nwy)[:, None, None] * ws - pad + (key // wse)[None, None, :]
    xx = torch.arange(nwx)[None, :, None] * ws - pad + (key % wse)[None, None, :]
    y, xx = y.expand(nwy, nwx, -1), xx.expand(nwy, nwx, -1)
    inside = (y >= 0) & (y < h) & (xx >= 0) & (xx < w)
    vals = x[:, y.clamp(0, h - 1), xx.clamp(0, w - 1)]
    return vals * inside.reshape((1, nwy, nwx, wse * wse) + (1,) * (x.dim() - 3)).to(x.dtype), inside


def ref_keybias(score_map, k, ws: int, wse: int, pad: int, k_keep: int, score_dtype=torch.float64):
    """hat_ocab_keybias.  score_map: (B,H,W) saliency (focus mode) or None (norm mode: the score is ||k||_2 over the channels of
    k (B,H,W,C)).  Returns kb (B, nWy, nWx, round_up(wse^2, 16)) fp64 — the score for a kept key (0 in norm mode), -inf for a
    pruned one, 0 in the dead tail past wse^2 — and keep (B, nWy, nWx, wse^2) bool.  Kept = the first k_keep keys of a STABLE
    descending sort of the scores (the lowest key index wins ties); keys outside the image score tanh(0) = 0 / norm 0.
    score_dtype float32 ranks on float32(tanh_fp64(sal)): the precision the kernel holds its scores in."""
    nk = wse * wse
    nkp = (nk + 15) // 16 * 16
    if score_map is not None:
        score = torch.tanh(key_windows(score_map.double(), ws, wse, pad)[0]).to(score_dtype).double()
    else:
        score = key_windows(k.double(), ws, wse, pad)[0].pow(2).sum(-1).sqrt()
    order = torch.argsort(-score, dim=-1, stable=True)
    keep = torch.zeros_like(score, dtype=torch.bool).scatter_(-1, order[..., :min(k_keep, nk)], True)
    kept_val = score if score_map is not None else torch.zeros_like(score)
    kb = torch.zeros(score.shape[:-1] + (nkp,), dtype=torch.float64)
    kb[..., :nk] = torch.where(keep, kept_val, torch.full_like(score, float("-inf")))
    return kb, keep


def ref_attention_kb(q, k, v, table, rpi, ws: int, wse: int, heads: int, kb):
    """hat_ocab_attention_kb in fp64.  q (already scaled), k, v: (B,H,W,C); table ((ws+wse-1)^2, heads) and rpi (ws^2, wse^2) as
    the reference holds them (negative indices wrap); kb (B, nWy, nWx, >= wse^2): the logit of a key with kb = -inf is REPLACED
    by -1e4, otherwise kb is added; then the relative-position bias, then softmax.  Entries of kb past wse^2 are ignored."""
    b, h, w, c = q.shape
    d, nk = c // heads, wse * wse
    nwy, nwx = h // ws, w // ws
    pad = (wse - ws + 1) // 2
    q, k, v, kb = q.double(), k.double(), v.double(), kb.double()[..., :nk]
    qw = q.reshape(b, nwy, ws, nwx, ws, heads, d).permute(0, 1, 3, 5, 2, 4, 6).reshape(b, nwy, nwx, heads, ws * ws, d)
    bias = table.double()[rpi.reshape(-1)].reshape(ws * ws, nk, heads).permute(2, 0, 1)
    out = torch.empty(b, h, w, c, dtype=torch.float64)
    for i in range(b):      # one sample at a time: the logits of a 16 -> 25 window are 256 x 625 per head
        kw_ = key_windows(k[i:i + 1], ws, wse, pad)[0][0].reshape(nwy, nwx, nk, heads, d).permute(0, 1, 3, 2, 4)
        vw_ = key_windows(v[i:i + 1], ws, wse, pad)[0][0].reshape(nwy, nwx, nk, heads, d).permute(0, 1, 3, 2, 4)
        logit = qw[i] @ kw_.transpose(-2, -1)                                   # (nWy, nWx, heads, ws^2, nk)
        kbi = kb[i][:, :, None, None, :]
        logit = torch.where(torch.isneginf(kbi), torch.full_like(logit, -1e4), logit + torch.nan_to_num(kbi, neginf=0.0))
        o = torch.softmax(logit + bias, dim=-1) @ vw_                           # (nWy, nWx, heads, ws^2, d)
        out[i] = o.reshape(nwy, nwx, heads, ws, ws, d).permute(0, 3, 1, 4, 2, 5).reshape(h, w, c)
    return out


def ref_sgfn_gate(u, wdw, bdw, half: int):
    """hat_sgfn_gate in fp64.  u (B,H,W,2*half); wdw (half,1,3,3), bdw (half,): out = [dw3x3(u[..., :half]) * silu(u[..., half:]) |
    u[..., half:]], (B,H,W,2*half)."""
    u = u.double()
    a = F.conv2d(u[..., :half].permute(0, 3, 1, 2), wdw.double(), bdw.double(), padding=1, groups=half).permute(0, 2, 3, 1)
    g = u[..., half:]
    return torch.cat([a * (g / (1.0 + torch.exp(-g))), g], dim=-1)
