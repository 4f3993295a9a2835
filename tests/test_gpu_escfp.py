"""ESCFP on the device: the four hat_escfp_* kernels and the shared kernels at their new shapes (3 heads, 48 -> 144, 48 -> 48) against
fp64 restatements of the same operation on the kernels' own inputs (tests/esc_ref.py, tests/escfp_ref.py), the whole model against
the reference's goldens (tests/golden/escfp_*.npz, gen_golden_escfp.py), batches against single frames, eager against graph replay,
and a reference-style option file through `python -m super_resolution_amd.test`.

Bars: fp32 1e-4 max-abs (the project's fp32 bar) for kernels, intermediates and outputs.  bf16 kernels: helpers.check's bar.  bf16
whole model: per case the reference's own bf16-vs-fp32 PSNR rounded down to a whole dB and capped at 40, and its max-abs x 1.25, both
recorded in escfp_surface.json by the generator."""
import math

import pytest
import torch
import torch.nn.functional as F

import esc_ref as E
import escfp_ref as R
from helpers import check, max_abs, q, rnd
from oracle import hat_oracle as O
from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

MAP = (20, 37)   # 3 x 4 tiles of 8 x 12: ragged in both axes, the last tile column is one pixel wide
C = 48


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rows(x_bchw, ld, tdt, dev, fill=7.0):
    """(B,C,H,W) -> device (B, H*W, ld) rows of dtype tdt whose pad channels hold `fill` (nothing may read them)."""
    b, c, h, w = x_bchw.shape
    out = torch.full((b, h * w, ld), fill, dtype=tdt, device=dev)
    out[:, :, :c] = x_bchw.reshape(b, c, h * w).permute(0, 2, 1).to(dev).to(tdt)
    return out


def _maps(rows, c, h, w):
    return rows[:, :, :c].float().cpu().permute(0, 2, 1).reshape(rows.shape[0], c, h, w)


def _pads_untouched(rows, c):
    return rows.shape[2] == c or float((rows[:, :, c:].float() - 7.0).abs().max()) == 0.0


def _ffn_sd(hid, dtype, b1_mean=0.0):
    """Seeded 48-channel ConvFFN parameters under the prefix "f", the MFMA operands rounded to dtype."""
    k = f"efp{hid}"
    return {"f.proj.weight": q(rnd(k + "w1", (hid, C, 1, 1), std=C ** -0.5), dtype), "f.proj.bias": rnd(k + "b1", (hid,), std=0.1) + b1_mean,
            "f.dwc.weight": rnd(k + "dw", (hid, 1, 3, 3), std=1 / 3), "f.dwc.bias": rnd(k + "db", (hid,), std=0.1),
            "f.aggr.weight": q(rnd(k + "w2", (C, hid, 1, 1), std=hid ** -0.5), dtype), "f.aggr.bias": rnd(k + "b2", (C,), std=0.1)}


def _convffn(dtype, hid, full, dev, B=1, b1_mean=0.0, out_f32=False):
    """hat_escfp_convffn once on the 20x37 map; full: with the LayerNorm, the residual and the pool.  -> (out maps, fp64 reference,
    partials or None, raw out rows)."""
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = torch.float32 if out_f32 else ops.TORCH_DTYPE[dt]
    h, w = MAP
    sd = _ffn_sd(hid, dtype, b1_mean)
    pf = ops.pack_escfp_convffn(sd, "f", dt, dev)
    x, r = rnd(f"x{hid}", (B, C, h, w)), rnd(f"r{hid}", (B, C, h, w))
    g, b = rnd("lng", (C,), std=0.1) + 1.0, rnd("lnb", (C,), std=0.1)
    ldx, ldr, ldo = 52, 56, 56   # (52 % 8 != 0: fp32 rows only; T rows need a multiple of 16 bytes)
    xr, rr = _rows(x, ldx, torch.float32, dev), _rows(r, ldr, torch.float32, dev)
    out = torch.full((B, h * w, ldo), 7.0, dtype=tdt, device=dev)
    parts = torch.full((B, ops.esc_convffn_tiles(h, w), 16), 7.0, device=dev) if full else None
    ops.escfp_convffn(pf, xr, out, B=B, H=h, W=w, dtype=dt, ln=(g.to(dev), b.to(dev)) if full else None, eps=R.LN_EPS,
                      r=rr if full else None, partials=parts, ldx=ldx, ldr=ldr, ldo=ldo)
    torch.cuda.synchronize()
    sd64 = E.d64(sd)
    n = E.layernorm(x.double(), g.double(), b.double()) if full else x.double()
    ref = E.convffn(n, sd64, "f") + (r.double() if full else 0.0)
    assert _pads_untouched(out, C), "pad channels written"
    return _maps(out, C, h, w), ref, parts, out


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("full", [False, True], ids=["plain", "ln+r+pool"])
@pytest.mark.parametrize("hid", [60, 72, 96])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_convffn_matches_fp64(dtype, hid, full, B):
    dev = _dev()
    from super_resolution_amd import ops
    assert ops.esc_convffn_tiles(*MAP) == 12
    got, ref, parts, raw = _convffn(dtype, hid, full, dev, B=B)
    check(got, ref, dtype, f"hat_escfp_convffn hid {hid}", f32_tol=1e-4)
    if full:
        # the pool partials are the sums of the stored values of channels 0..15 over each tile's pixels
        stored = got[:, :16].double()
        want = torch.stack([stored[:, :, ty:ty + 8, tx:tx + 12].sum((2, 3)) for ty in range(0, 20, 8) for tx in range(0, 37, 12)], 1)
        assert parts.shape == (B, 12, 16)
        err = float((parts.double().cpu() - want).abs().max())
        assert err <= 1e-4 * max(1.0, float(want.abs().max())), err
        got2, _, parts2, raw2 = _convffn(dtype, hid, full, dev, B=B)
        assert torch.equal(raw, raw2) and torch.equal(parts, parts2), "two runs differ"


def test_convffn_fp32_output_rows_from_the_bf16_instantiation():
    dev = _dev()
    got, ref, _, _ = _convffn("bf16", 60, True, dev, out_f32=True)
    check(got, ref, "bf16", "hat_escfp_convffn bf16 -> fp32 rows")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_convffn_zero_pads_h_not_x(dtype):
    """The depthwise conv pads h with zeros.  With a proj bias around 1, gelu(b1) outside the image would move the border pixels
    by O(1): the kernel must match the zero-padding restatement and be far from the other one."""
    dev = _dev()
    got, ref, _, _ = _convffn(dtype, 60, False, dev, b1_mean=1.0)
    check(got, ref, dtype, "hat_escfp_convffn, zero-padded h", f32_tol=1e-4)
    sd64 = E.d64(_ffn_sd(60, dtype, 1.0))
    x = rnd("x60", (1, C) + MAP).double()
    xp = F.pad(x, (1, 1, 1, 1))   # x zero-padded instead: h outside the image becomes gelu(b1)
    hp = E.gelu(F.conv2d(xp, sd64["f.proj.weight"], sd64["f.proj.bias"]))
    h2 = E.gelu(F.conv2d(hp, sd64["f.dwc.weight"], sd64["f.dwc.bias"], groups=60)) + hp[:, :, 1:-1, 1:-1]
    wrong = F.conv2d(h2, sd64["f.aggr.weight"], sd64["f.aggr.bias"])
    assert max_abs(wrong, ref) > 0.1 and max_abs(got[:, :, 0], wrong[:, :, 0]) > 0.1


def test_convffn_refuses_bad_arguments():
    dev = _dev()
    from super_resolution_amd import ops
    pf = ops.pack_escfp_convffn(_ffn_sd(60, "f32"), "f", ops.HAT_F32, dev)
    x = torch.zeros(1, 20 * 37, C, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.escfp_convffn(pf, x, x, B=1, H=20, W=37, dtype=ops.HAT_F32)            # in place: the halo would read written rows
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.escfp_convffn(pf, x, torch.zeros_like(x), B=1, H=20, W=37, dtype=ops.HAT_F32, ldx=44)
    pf.hid_p = 128
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.escfp_convffn(pf, x, torch.zeros_like(x), B=1, H=20, W=37, dtype=ops.HAT_F32)


@pytest.mark.parametrize("npix", [35, 16 * 4096 * 2 + 35], ids=["35px", "3trips"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_layernorm_eps_pads_and_grid_trips(dtype, npix):
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    x = rnd(f"lnx{npix}", (1, C, 1, npix), std=1e-3)   # small rows: eps 1e-6 against 1e-5 is a visible difference
    g, b = rnd("lng", (C,), std=0.1) + 1.0, rnd("lnb", (C,), std=0.1)
    xr = _rows(x, 52, torch.float32, dev)
    y = torch.full((1, npix, 56), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.escfp_layernorm(xr, y, g.to(dev), b.to(dev), npix=npix, dtype=dt, eps=1e-6, ldx=52, ldy=56)
    ref = E.layernorm(x.double(), g.double(), b.double(), 1e-6)
    check(_maps(y, C, 1, npix), ref, dtype, "hat_escfp_layernorm", f32_tol=1e-4)
    assert _pads_untouched(y, C), "pad channels written"
    assert max_abs(E.layernorm(x.double(), g.double(), b.double(), 1e-5), ref) > 0.1
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.escfp_layernorm(xr, y, g.to(dev), b.to(dev), npix=npix, dtype=dt, eps=1e-6, ldx=44, ldy=56)


# ---- the large-kernel branch ------------------------------------------------------------------------------------------------
def _lk_sd():
    return {"p.plk.proj.1.weight": rnd("lkw1", (4, 16, 1, 1), std=0.25), "p.plk.proj.1.bias": rnd("lkb1", (4,), std=0.1),
            "p.plk.proj.3.weight": rnd("lkw2", (144, 4, 1, 1), std=0.1), "p.plk.proj.3.bias": rnd("lkb2", (144,), std=0.02),
            "lk_channel": rnd("lkc", (16, 16, 1, 1), std=0.25), "lk_spatial": rnd("lks", (16, 1, 13, 13), std=1 / 13)}


def _weights(dtype, nblk, dev, B=2, N=777):
    """hat_escfp_weights on seeded partials -> (raw (B,16,kpad) output pre-filled with 7.0, the fp64 dense filter (B,16,16,13,13),
    the fp64 depthwise kernels K (B,16,13,13) it was folded from, the pack, the fp64 parameters)."""
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    sd = _lk_sd()
    lk = ops.pack_escfp_lk(sd, "p", dt, dev)
    parts = rnd(f"lkparts{nblk}", (B, nblk, 16), std=N / nblk)
    out = torch.full((B, 16, lk.kpad), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.escfp_weights(parts.to(dev), nblk, N, lk, out, B=B, dtype=dt)
    torch.cuda.synchronize()
    sd64 = E.d64(sd)
    mean = (parts.double().sum(1) / N).reshape(B, 16, 1, 1)
    dyn = F.conv2d(E.gelu(F.conv2d(mean, sd64["p.plk.proj.1.weight"], sd64["p.plk.proj.1.bias"])), sd64["p.plk.proj.3.weight"],
                   sd64["p.plk.proj.3.bias"]).reshape(B, 16, 3, 3)
    k = F.pad(dyn, (5, 5, 5, 5)) + sd64["lk_spatial"].reshape(1, 16, 13, 13)
    weff = sd64["lk_channel"].reshape(1, 16, 16, 1, 1) * k.reshape(B, 16, 1, 13, 13)
    return out, weff, k, lk, sd64


@pytest.mark.parametrize("nblk", [12, 700], ids=["12slots", "700slots_2trips"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weights_match_fp64(dtype, nblk):
    dev = _dev()
    out, weff, _, lk, _ = _weights(dtype, nblk, dev)
    # (one trip of the kernel's reduction loop covers 64 parts x 8 chains = 512 slots: 700 slots take two)
    got = out[:, :, :169 * 16].float().cpu().reshape(2, 16, 169, 16).permute(0, 1, 3, 2).reshape(2, 16, 16, 13, 13)   # K = 16 tap + ci
    check(got, weff, dtype, f"hat_escfp_weights {nblk} slots", f32_tol=1e-4)
    assert max_abs(weff[0], weff[1]) > 1e-3, "the two samples must have different dynamic kernels"
    assert out.shape[2] > 169 * 16 and float(out[:, :, 169 * 16:].float().abs().max()) == 0.0, "K past the data must be zero"
    out2, _, _, _, _ = _weights(dtype, nblk, dev)
    assert torch.equal(out, out2), "two runs differ"
    if dtype == "bf16":   # one rounding: the fp32 product rounded to bf16, not a product of rounded factors
        out32, _, _, _, _ = _weights("f32", nblk, dev)
        assert torch.equal(out[:, :, :169 * 16].float(), out32[:, :, :169 * 16].to(torch.bfloat16).float())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_conv13_fed_by_the_new_weights_equals_the_two_step_form(dtype):
    """hat_esc_conv13 (bf16) / hat_conv k = 13 with per-sample weights (fp32) on hat_escfp_weights' image, against the reference's
    conv1x1(lk_channel) + depthwise 13x13 with each sample's own kernel, on 20x37, B = 2."""
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    h, w = MAP
    out, _, k, lk, sd64 = _weights(dtype, 12, dev)
    z = q(rnd("lkz", (2, C, h, w)), dtype)
    zr = _rows(z, C, tdt, dev)
    y16 = torch.full((2, h * w, 16), 7.0, dtype=tdt, device=dev)
    if ops.esc_conv13_supported(16, 13, dt):
        assert dtype == "bf16"
        ops.esc_conv13(zr, out, y16, B=2, H=h, W=w, ldx=C, kpad=lk.kpad, dtype=dt)
    else:
        pw = ops.PackedConv(out, lk.zero_bias, 13, 16, lk.kpad, 1, 1, 16, w_bstride=16 * lk.kpad)
        ops.conv(pw, zr, y16, B=2, H=h, W=w, dtype=dt, ldx=C, ldo=16, n_store=16)
    torch.cuda.synchronize()
    z1 = z[:, :16].double()
    t = F.conv2d(z1, sd64["lk_channel"])
    ref = torch.cat([F.conv2d(t[b:b + 1], k[b].reshape(16, 1, 13, 13), padding=6, groups=16) for b in range(2)])
    check(_maps(y16, 16, h, w), ref, dtype, "13x13 conv on hat_escfp_weights' image", f32_tol=1e-4)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (33, 40)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_shuffle_bicubic_matches_torch(s, hw):
    dev = _dev()
    from super_resolution_amd import ops
    h, w = hw
    ld = (3 * s * s + 3) // 4 * 4
    rows, img = rnd(f"sb{s}{hw}", (2, 3 * s * s, h, w)), synth.uniform(5, f"sbx{hw}", (2, 3, h, w))
    out = torch.zeros(2, 3, h * s, w * s, device=dev)
    ops.escfp_shuffle_bicubic(_rows(rows, ld, torch.float32, dev), img.to(dev), ops.bicubic_phase_table(s).to(dev), out, B=2, H=h, W=w, s=s, ld=ld)
    want = F.pixel_shuffle(rows, s) + F.interpolate(img, scale_factor=s, mode="bicubic")
    err = max_abs(out.cpu(), want)
    assert err <= 1e-4, f"x{s} {hw}: max-abs {err:.3e}"
    if hw == (33, 40):
        base = out.cpu() - F.pixel_shuffle(rows, s)
        assert float(base.min()) < -0.01 and float(base.max()) > 1.01, "the bicubic base overshoots [0, 1] and is not clamped"


def test_shuffle_bicubic_refusals():
    dev = _dev()
    from super_resolution_amd import ops
    rows, img, out = torch.zeros(1, 6, 76, device=dev), torch.zeros(1, 3, 2, 3, device=dev), torch.zeros(1, 3, 10, 15, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.escfp_shuffle_bicubic(rows, img, torch.zeros(5, 4, device=dev), out, B=1, H=2, W=3, s=5, ld=76)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.escfp_shuffle_bicubic(rows, img, torch.zeros(2, 4, device=dev), out, B=1, H=2, W=3, s=2, ld=8)


# ---- existing kernels at the new shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(40, 72), (33, 64)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_window_attention_r_with_three_heads(dtype, hw):
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    h, w = hw
    qkv = q(rnd(f"qkv3{hw}", (1, 3 * C, h, w)), dtype)
    table = rnd("rpb32x3", (3, 63 * 63), std=0.5)
    rows = _rows(qkv, 3 * C, tdt, dev)
    rows[:, :, :C] = (rows[:, :, :C].float() * 0.25).to(tdt)   # q pre-multiplied by head_dim^-0.5: a power of two, exact
    ldo = 52 if dtype == "f32" else 56
    out = torch.full((1, h * w, ldo), 7.0, dtype=tdt, device=dev)
    ops.window_attention_r(rows, rows.view(-1)[C:], table.to(dev), out, B=1, h=h, w=w, C_=C, heads=3, ws=32, ldq=3 * C, ldkv=3 * C, ldo=ldo,
                           dtype=dt)
    torch.cuda.synchronize()
    Hp, Wp = -(-h // 32) * 32, -(-w // 32) * 32
    padded = qkv.double()[:, :, E.reflect_index(h, Hp)][:, :, :, E.reflect_index(w, Wp)]
    ref = E.attention_core(padded, table.double(), 32, 3)[:, :, :h, :w]
    check(_maps(out, C, h, w), ref, dtype, f"hat_window_attention_r 3 heads {hw}", f32_tol=1e-4)
    assert _pads_untouched(out, C), "pad channels written"


def _pointwise(pw, x, out, dt, geo, **kw):
    from super_resolution_amd import ops
    (ops.linear if pw.frag else ops.conv)(pw, x, out, **geo, dtype=dt, **kw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_to_qkv_48_to_144_and_aggr_48_to_48_with_split_input(dtype):
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    h, w = 21, 19
    geo = dict(B=1, H=h, W=w)
    x = q(rnd("pwx", (1, C, h, w)), dtype)
    xr = _rows(x, C, tdt, dev)
    wq, bq = q(rnd("pwq", (3 * C, C), std=C ** -0.5), dtype), rnd("pwqb", (3 * C,), std=0.1)
    out = torch.zeros(1, h * w, 3 * C, dtype=tdt, device=dev)
    _pointwise(ops.pack_pointwise(wq, bq, dt, dev), xr, out, dt, geo, ldx=C, ldo=3 * C)
    check(_maps(out, 3 * C, h, w), F.conv2d(x.double(), wq.double()[:, :, None, None], bq.double()), dtype, "to_qkv 48 -> 144", f32_tol=1e-4)
    # aggr: channels 0..15 from the compact 13x13 output, 16..47 from z, plus the fp32 residual, fp32 rows out
    wa, ba = q(rnd("pwa", (C, C), std=C ** -0.5), dtype), rnd("pwab", (C,), std=0.1)
    y16, r1 = q(rnd("pwy", (1, 16, h, w)), dtype), rnd("pwr", (1, C, h, w))
    pa = ops.pack_pointwise(wa, ba, dt, dev)
    assert pa.frag, "48 -> 48 runs on hat_linear"
    o32 = torch.zeros(1, h * w, C, device=dev)
    _pointwise(pa, xr, o32, dt, geo, ldx=C, ldo=C, out_mode=ops.O_NHWC_F32, x0=_rows(y16, 16, tdt, dev), c_split=16, ldx0=16,
               r1=_rows(r1, C, torch.float32, dev), ldr1=C)
    ref = F.conv2d(torch.cat([y16, x[:, 16:]], 1).double(), wa.double()[:, :, None, None], ba.double()) + r1.double()
    check(_maps(o32, C, h, w), ref, dtype, "aggr 48 -> 48, x0 / c_split 16, r1", f32_tol=1e-4)


# ---- whole model ------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name, dtype, dev):
    """The ESCFP of golden case `name` with its seeded weights ('d': case a's x2 checkpoint in a x4 model)."""
    from super_resolution_amd.registry import build_network
    if (name, dtype) not in _NETS:
        cfg, sd, g, meta = R.load_case(name)
        net = build_network(dict(cfg, type="ESCFP", attn_type="Naive", compute_dtype=dtype)).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[(name, dtype)] = (net.to(dev), g, meta)
    return _NETS[(name, dtype)]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_whole_model_fp32_matches_reference(name):
    dev = _dev()
    net, g, _ = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    taps = {}
    y = net.engine(dev).forward(x, taps=taps).clone()
    if "tap_pixels" in g:   # the intermediates first, so that a failure points at a stage
        px = torch.from_numpy(g["tap_pixels"])
        for k in R.TAPS:
            err = max_abs(taps[k].cpu()[:, px, :C], g[k])
            print(f"escfp_{name} {k}: max-abs {err:.3e}")
            assert err <= 1e-4, f"escfp_{name} {k}: max-abs {err:.3e}"
    err = max_abs(y.cpu(), g["y"])
    print(f"escfp_{name} y: max-abs {err:.3e}")
    assert err <= 1e-4, f"escfp_{name}: max-abs {err:.3e}"
    assert torch.equal(net(x), y), "two eager forwards differ"


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_whole_model_bf16_within_the_reference_bf16_deviation(name):
    dev = _dev()
    net, g, meta = _net(name, "bf16", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    taps = {}
    y = net.engine(dev).forward(x, taps=taps).clone().cpu()
    if "tap_pixels" in g:
        px = torch.from_numpy(g["tap_pixels"])
        for k in R.TAPS:
            print(f"escfp_{name} bf16 {k}: max-abs {max_abs(taps[k].cpu()[:, px, :C], g[k]):.3e} on values up to {float(abs(g[k]).max()):.2f}")
    psnr, err = O.psnr_float(y, torch.from_numpy(g["y"])), max_abs(y, g["y"])
    bar_db, bar_abs = min(40.0, math.floor(meta["bf16"]["psnr"])), 1.25 * meta["bf16"]["max_abs"]
    print(f"escfp_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})")
    assert psnr >= bar_db and err <= bar_abs, f"escfp_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})"
    assert torch.equal(net(x).cpu(), y), "two eager forwards differ"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_each_sample_of_a_batch_equals_its_single_frame_forward(dtype):
    dev = _dev()
    net, g, _ = _net("c", dtype, dev)
    x = torch.from_numpy(g["x"]).to(dev)
    y = net(x)
    assert y.shape == (2, 3, 99, 120)
    for b in range(2):
        assert torch.equal(net(x[b:b + 1].contiguous())[0], y[b]), f"sample {b}"
    assert max_abs(y[0].cpu(), y[1].cpu()) > 0.1


def test_graph_replay_equals_eager_and_second_size():
    dev = _dev()
    net, g, _ = _net("a", "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    eager = net(x)
    net.use_graph = True
    try:
        assert torch.equal(net(x), eager) and torch.equal(net(x), eager)   # capture, then replay
        x2 = synth.synth_input(R.X_SEED, (1, 3, 33, 64)).to(dev)           # another size after 40x72: the workspace is keyed by shape
        cfg, sd, _, _ = R.load_case("a")
        want = R.forward(R.d64(sd), cfg, x2.cpu().double())
        assert max_abs(net(x2).cpu(), want) <= 1e-4
        assert torch.equal(net(x), eager)
    finally:
        net.use_graph = False
    assert max_abs(net(x2).cpu(), want) <= 1e-4 and torch.equal(net(x), eager)


def test_small_frames_are_refused_and_the_not_built_paths_raise():
    dev = _dev()
    net, _, _ = _net("a", "fp32", dev)
    with pytest.raises(RuntimeError, match="reflect-padded"):
        net(torch.zeros(1, 3, 16, 40, device=dev))
    with pytest.raises(RuntimeError, match="reflect-padded"):
        net(torch.zeros(2, 3, 40, 16, device=dev))
    x = torch.zeros(1, 3, 40, 40, device=dev)
    for call in (lambda: net.forward_ensemble(x), lambda: net.forward_to_u8(x), lambda: net.forward_yuv420(x), lambda: net.forward_bands(x, 2),
                 lambda: net.forward_band_parallel(x)):
        with pytest.raises(NotImplementedError, match="runs its float forward only"):
            call()
    from super_resolution_amd.registry import build_network
    with pytest.raises(ValueError, match="not supported"):   # ESC itself keeps refusing 48 channels
        build_network(dict(R.CASES["a"][0], type="ESC", use_ln=True)).to(dev).eval()(x)


def test_reference_style_yaml_through_the_test_entry(tmp_path):
    """An option file as the reference ships them (ESC_FP_X4.yaml: model_type ESRModel, network_g.type ESCFP) through `python -m
    super_resolution_amd.test`: the PSNR is the one metrics.py gives for the fp32 golden path's output (tests/escfp_ref.py in fp32
    on the host), within 1e-3 dB."""
    dev = _dev()
    import yaml
    from super_resolution_amd import data as D, metrics as M, test as T
    cfg, sd, _, _ = R.load_case("b")
    torch.save({"params_ema": sd}, tmp_path / "net.pth")
    sizes = [(40, 45), (36, 50)]
    for i, (h, w) in enumerate(sizes):
        D.write_image(M.tensor2img(synth.synth_input(30 + i, (1, 3, h, w))), str(tmp_path / "lq" / f"im{i}.png"))
        D.write_image(M.tensor2img(synth.synth_input(40 + i, (1, 3, 4 * h, 4 * w))), str(tmp_path / "gt" / f"im{i}.png"))
    opt = {"name": "ESC_FP_toy_X4", "model_type": "ESRModel", "scale": 4, "num_gpu": 1, "manual_seed": 0,
           "datasets": {"test_1": {"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"),
                                   "dataroot_lq": str(tmp_path / "lq"), "io_backend": {"type": "disk"}}},
           "network_g": dict(cfg, type="ESCFP", attn_type="Flex", compute_dtype="fp32"),
           "path": {"pretrain_network_g": str(tmp_path / "net.pth"), "strict_load_g": True, "param_key_g": "params_ema",
                    "visualization": str(tmp_path / "vis")},
           "val": {"save_img": False, "suffix": None, "metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": True}}}}
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    res = T.main(["-opt", str(tmp_path / "opt.yml")])
    assert len(res["Toy"]["images"]) == 2
    for i, (h, w) in enumerate(sizes):
        lq = D.read_image(str(tmp_path / "lq" / f"im{i}.png")).unsqueeze(0)
        xp = F.pad(lq, (0, (-w) % 32, 0, (-h) % 32), "reflect")
        y = R.forward(sd, cfg, xp)[:, :, :4 * h, :4 * w]
        gt8 = M.tensor2img(D.read_image(str(tmp_path / "gt" / f"im{i}.png")))
        want = M.calculate_metric({"img": M.tensor2img(y), "img2": gt8}, opt["val"]["metrics"]["psnr"])
        assert res["Toy"]["images"][i]["psnr"] == pytest.approx(want, abs=1e-3)
