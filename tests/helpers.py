"""Shared helpers for the tests: golden loading, oracle nets with synthetic weights, the per-kernel GPU tests' input / tolerance
helpers, plain fp64 restatements of the HATX attention options and the SGFN gate that take the kernels' own inputs, and the
builders / references of the multi-trip tests (test_gpu_multitrip.py): device-drawn activations, a banded fp64 convolution,
the chunked re-run of a pointwise launch.  (The hat_window_attention cases and their restatement are in wmsa_cases.py.)"""
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


def fill_rows(x_bhwc: torch.Tensor, ld: int, tdt, dev, fill, c_zero=None):
    """(B,H,W,C) float -> device (B, H*W, ld) of dtype tdt whose pad channels hold `fill` (nothing may read them).  c_zero: channels
    [C, c_zero) are zero instead (hat_conv's documented zero pad up to Cin_p, which it may read under zero weights)."""
    b, h, w, c = x_bhwc.shape
    out = torch.full((b, h * w, ld), fill, dtype=tdt, device=dev)
    out[:, :, :c] = x_bhwc.reshape(b, h * w, c).to(dev).to(tdt)
    if c_zero is not None and c_zero > c:
        out[:, :, c:c_zero] = 0
    return out


def pads_keep(rows: torch.Tensor, c: int, fill: float, what: str):
    """The pad channels [c, ld) of (B, N, ld) rows pre-filled with `fill` still hold it, bit for bit: the launch wrote live columns only."""
    assert rows.shape[-1] > c, what + ": no pad channels"
    assert torch.equal(rows[..., c:], torch.full_like(rows[..., c:], fill)), what + ": pad channels written"


def check(got: torch.Tensor, ref: torch.Tensor, dtype: str, what: str, f32_tol=2e-5):
    got, ref = got.detach().double(), ref.detach().double()
    if got.device != ref.device:      # (two tensors of one device are judged there: the multi-trip tests' maps are 0.2 Mpx)
        got, ref = got.cpu(), ref.cpu()
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


def esc_ffn_sd(hid, dtype, b1_mean=0.0):
    """Seeded ConvFFN parameters under the prefix "f" (esc_ref.convffn / ops.pack_esc_convffn), the MFMA operands rounded to dtype."""
    k = f"ecf{hid}"
    return {"f.proj.weight": q(rnd(k + "w1", (hid, 64, 1, 1), std=1 / 8), dtype), "f.proj.bias": rnd(k + "b1", (hid,), std=0.1) + b1_mean,
            "f.dwc.weight": rnd(k + "dw", (hid, 1, 3, 3), std=1 / 3), "f.dwc.bias": rnd(k + "db", (hid,), std=0.1),
            "f.aggr.weight": q(rnd(k + "w2", (64, hid, 1, 1), std=hid ** -0.5), dtype), "f.aggr.bias": rnd(k + "b2", (64,), std=0.1)}


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


# ------------------------------------------------------------------------------------------------
# multi-trip tests (test_gpu_multitrip.py): frames of 0.1 - 0.5 Mpx, so activations are drawn on the device (synth.normal is host
# numpy in float64) and the references run in fp64 where the operands already are
# ------------------------------------------------------------------------------------------------
def dev_randn(key: str, shape, dev, std=1.0, mean=0.0):
    """fp32 N(mean, std^2) of `shape` drawn on `dev` from a generator seeded by `key` (the same tensor for the same key within a
    run: the big launch, its chunked re-run and the reference all read one buffer)."""
    g = torch.Generator(device=dev)
    g.manual_seed(synth._fnv1a64(key) & 0x7FFFFFFFFFFF)
    return torch.randn(tuple(shape), generator=g, device=dev) * std + mean


def dev_rows(key: str, B: int, N: int, C_: int, ld: int, tdt, dev, std=1.0, mean=0.0):
    """(B, N, ld) rows of dtype tdt on the device: N(mean, std^2) in the first C_ channels, zero pad channels (to_dev's layout)."""
    out = torch.zeros(B, N, ld, dtype=tdt, device=dev)
    out[:, :, :C_] = dev_randn(key, (B, N, C_), dev, std, mean).to(tdt)
    return out


def conv_ref_banded(x: torch.Tensor, w: torch.Tensor, bias=None, band: int = 64):
    """fp64 'same' convolution (stride 1, zero padding) of a channel-last map, on x's device: x (B, H, W, Cin); w (Cout, Cin, k, k)
    or per-sample (B, Cout, Cin, k, k); -> (B, H, W, Cout) fp64.  Row bands of `band` rows with a k // 2 halo, one matmul per tap:
    only a band of the map exists in fp64 next to the result, and no convolution library is involved."""
    b, h, wd, cin = x.shape
    k, pad, cout = w.shape[-1], w.shape[-1] // 2, w.shape[-4]
    w = w.double().to(x.device)
    out = torch.empty(b, h, wd, cout, dtype=torch.float64, device=x.device)
    for y0 in range(0, h, band):
        y1 = min(y0 + band, h)
        lo, hi = max(y0 - pad, 0), min(y1 + pad, h)
        xb = F.pad(x[:, lo:hi].double(), (0, 0, pad, pad, pad - (y0 - lo), pad - (hi - y1)))     # (B, rows + 2 pad, W + 2 pad, Cin)
        acc = torch.zeros(b, (y1 - y0) * wd, cout, dtype=torch.float64, device=x.device)
        for dy in range(k):
            for dx in range(k):
                acc += xb[:, dy:dy + (y1 - y0), dx:dx + wd].reshape(b, -1, cin) @ w[..., dy, dx].transpose(-1, -2)
        out[:, y0:y1] = acc.reshape(b, y1 - y0, wd, cout)
    return out if bias is None else out + bias.double().to(x.device)


def run_chunked(launch, rows: dict, B: int, N: int, chunk: int):
    """Re-run a pointwise launch over consecutive chunks of at most `chunk` pixels that never cross a sample: launch(views, b) gets
    the (1, n, ld) views of every per-pixel tensor in `rows` ((B, N, ld), contiguous) and the sample index, and launches
    B = 1, H = 1, W = n on them."""
    for b in range(B):
        for p0 in range(0, N, chunk):
            p1 = min(p0 + chunk, N)
            launch({key: t[b:b + 1, p0:p1] for key, t in rows.items()}, b)


def need_trips(units: int, cap: int, depth: int, what: str):
    """Some loops take ceil(units / cap) >= depth trips, the others exactly one fewer (and at least one)."""
    hi, lo = -(-units // cap), units // cap
    assert hi >= depth and lo == hi - 1 and lo >= 1, f"{what}: {units} units on a first trip of {cap}: {hi} / {lo} trips, {depth} wanted"
    return hi, lo


def esc_weights_case(ops, dev, dtype: str, pdim: int, ks: int, nblk: int, B: int = 2, N: int = 777):
    """hat_esc_weights on seeded GAP partials of `nblk` blocks -> (the kernel's weights un-packed to (B, pdim, pdim, ks, ks) on
    the host, their fp64 restatement, the raw (B, npad, kpad) output pre-filled with 7.0, npad)."""
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    npad = 16 if pdim <= 16 else 32   # weight rows per sample and floats per GAP block
    gap = rnd("gp", (B, nblk, npad), std=1.0)
    gap[:, :, pdim:] = 0
    w1, b1 = rnd("w1", (pdim // 2, pdim), std=0.3), rnd("b1", (pdim // 2,), std=0.1)
    w2, b2 = rnd("w2", (pdim * 9, pdim // 2), std=0.3), rnd("b2", (pdim * 9,), std=0.1)
    plk = rnd("plk", (pdim, pdim, ks, ks), std=0.05)
    p = gap.double().sum(1)[:, :pdim] / N
    h = F.gelu(p @ w1.double().t() + b1.double())
    dk = (h @ w2.double().t() + b2.double()).reshape(B, pdim, 3, 3)
    weff = plk.double()[None].repeat(B, 1, 1, 1, 1)
    c = ks // 2
    for i in range(pdim):
        weff[:, i, i, c - 1:c + 2, c - 1:c + 2] += dk[:, i]
    lk = ops.pack_conv_weight(plk, None, ops.HAT_F32, dev, nt=1)
    kc = ops.KC[dt] * 3
    kpad = -(-(ks * ks * _r8(pdim)) // kc) * kc
    plkp = torch.zeros(npad, kpad, device=dev)
    plkp[:lk.w.shape[0], :min(kpad, lk.kpad)] = lk.w[:npad, :min(kpad, lk.kpad)]
    wout = torch.full((B, npad, kpad), 7.0, dtype=tdt, device=dev)
    ops.esc_weights(gap.to(dev), nblk, N, w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), plkp, wout, B=B, pdim=pdim, ksize=ks,
                    kpad=kpad, dtype=dt)
    torch.cuda.synchronize()
    cin_p = _r8(pdim)
    got = wout.float().cpu()[:, :pdim, :ks * ks * cin_p].reshape(B, pdim, ks, ks, cin_p)[..., :pdim].permute(0, 1, 4, 2, 3)
    return got, weff, wout, npad
