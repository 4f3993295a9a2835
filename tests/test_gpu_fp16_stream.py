"""The residual stream as FP16 rows through a whole residual group: the group conv (hat_conv, HatConvDesc.reserved0), the OCAB
projection (hat_linear, same bits) and the OCAB MLP (hat_ocab_mlp, out_f32 == 2) take r1 and / or write their fp32 result as
FP16 rows.  The arithmetic is the fp32-stream kernel's, only the load / store differ — FP16 in is exact, FP16 out is the
round-to-nearest of the same fp32 result, clamped to +-65504 — so on FP16-representable inputs every type combination must
agree BIT FOR BIT with the fp32 launch (the fused LayerNorm rows, GAP partials and compact copy come from the unrounded value).
Pattern: test_gpu_ops.test_hab_tail3_fp16_residual_rows."""
import pytest
import torch

from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

C = 144
COMBOS = [(False, False), (True, False), (False, True), (True, True)]   # (r1 FP16, out FP16)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(key, shape, std=1.0):
    return synth.normal(17, key, shape, std=std)


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _stream(key, B, N, dev):
    """an FP16-representable residual stream (B, N, C) as FP16 rows on the device"""
    return (rnd(key, (B, N, C), std=1.5) + 0.3).half().to(dev).contiguous()


@pytest.mark.parametrize("geom", [(2, 24, 40), (1, 19, 27)], ids=["B2_24x40", "ragged_19x27"])
def test_group_conv_fp16_stream(geom):
    """hat_conv, group-conv shape (3x3, 144 -> 144, bf16 rows in) with the fused LayerNorm, GAP partials and n16 copy; in place
    (r1 == out) when both sides have the same type, as the engine runs it."""
    from super_resolution_amd import ops
    B, H, W = geom
    dev, dt, N = _dev(), ops.HAT_BF16, geom[1] * geom[2]
    pw = ops.pack_conv_weight(bf(rnd("gw", (C, C, 3, 3), std=(9 * C) ** -0.5)), rnd("gb", (C,), std=0.1), dt, dev)
    assert pw.nt == 9 and pw.n_slices == 1
    x = bf(rnd("gx", (B, N, C))).to(torch.bfloat16).to(dev).contiguous()
    r16 = _stream("gr", B, N, dev)
    lg, lb = (1 + rnd("lg", (C,), std=0.1)).to(dev), rnd("lb", (C,), std=0.1).to(dev)
    tiles = ops.conv_tiles(pw, H, W, dt)
    res = {}
    for key in COMBOS + [("inplace", True), ("inplace", False)]:
        inplace = key[0] == "inplace"
        r_half, o_half = (key[1], key[1]) if inplace else key
        r1 = r16.clone() if r_half else r16.float()
        out = r1 if inplace else torch.full((B, N, C), 7.0, dtype=(torch.float16 if o_half else torch.float32), device=dev)
        n = torch.zeros(B, N, C, dtype=torch.bfloat16, device=dev)
        gap = torch.zeros(B, tiles, 16, device=dev)
        n16 = torch.zeros(B, N, 16, dtype=torch.bfloat16, device=dev)
        ops.conv(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, x_mode=ops.X_NHWC_T, out_mode=ops.O_NHWC_F32, r1=r1, ldr1=C,
                 ln=(lg, lb), ln_out=n, ld_ln=C, gap_out=gap, gap_c=16, n16_out=n16)
        torch.cuda.synchronize()
        res[key] = (out.cpu(), n.cpu(), gap.cpu(), n16.cpu())
    o0, n0, g0, s0 = res[(False, False)]
    assert torch.isfinite(o0).all() and float(o0.abs().max()) < 6e4
    for key, (o, n, gap, n16) in res.items():
        want = o0.half() if o.dtype == torch.float16 else o0
        assert torch.equal(o, want), f"output differs for {key}: max-abs {float((o.float() - want.float()).abs().max()):.3e}"
        assert torch.equal(n, n0) and torch.equal(gap, g0) and torch.equal(n16, s0), key
    # beyond the FP16 range: clamped to +-65504, not inf
    big = torch.full((1, 16 * 16, C), 7.0e4, device=dev)
    big[:, :, 1::2] = -7.0e4
    out = torch.zeros(1, 16 * 16, C, dtype=torch.float16, device=dev)
    ops.conv(pw, x[:1, :256].contiguous(), out, B=1, H=16, W=16, dtype=dt, ldx=C, ldo=C, x_mode=ops.X_NHWC_T,
             out_mode=ops.O_NHWC_F32, r1=big, ldr1=C)
    torch.cuda.synchronize()
    o = out.float().cpu()
    assert torch.equal(o[:, :, 0::2], torch.full_like(o[:, :, 0::2], 65504.0)) and torch.equal(o[:, :, 1::2], torch.full_like(o[:, :, 1::2], -65504.0))


@pytest.mark.parametrize("variant", ["ln16", "ln_ld148", "no_ln"])
@pytest.mark.parametrize("geom", [(2, 16, 40), (1, 19, 27)], ids=["B2_16x40", "ragged_19x27"])
def test_ocab_proj_fp16_stream(geom, variant):
    """hat_linear's OCAB-projection instantiation (144 -> 144, fp32 result + r1, fused LayerNorm with 16-byte rows, with rows
    that are not, and without it): every type combination of r1 / out, and in place as the engine runs it."""
    from super_resolution_amd import ops
    B, H, W = geom
    dev, dt, N = _dev(), ops.HAT_BF16, geom[1] * geom[2]
    pw = ops.pack_linear_weight(bf(rnd("pw", (C, C), std=C ** -0.5)), rnd("pb", (C,), std=0.1), dt, dev)
    assert pw.nt == 9 and pw.kpad // 32 == 5
    x = bf(rnd("px", (B, N, C))).to(torch.bfloat16).to(dev).contiguous()
    r16 = _stream("pr", B, N, dev)
    lg, lb = (1 + rnd("plg", (C,), std=0.1)).to(dev), rnd("plb", (C,), std=0.1).to(dev)
    ldn = 148 if variant == "ln_ld148" else C
    res = {}
    for key in COMBOS + [("inplace", True), ("inplace", False)]:
        inplace = key[0] == "inplace"
        r_half, o_half = (key[1], key[1]) if inplace else key
        r1 = r16.clone() if r_half else r16.float()
        out = r1 if inplace else torch.full((B, N, C), 7.0, dtype=(torch.float16 if o_half else torch.float32), device=dev)
        n = torch.zeros(B, N, ldn, dtype=torch.bfloat16, device=dev)
        lnkw = dict(ln=(lg, lb), ln_out=n, ld_ln=ldn) if variant != "no_ln" else {}
        ops.linear(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, out_mode=ops.O_NHWC_F32, r1=r1, ldr1=C, **lnkw)
        torch.cuda.synchronize()
        res[key] = (out.cpu(), n.cpu())
    o0, n0 = res[(False, False)]
    assert torch.isfinite(o0).all() and float(o0.abs().max()) < 6e4
    if variant != "no_ln":
        assert float(n0.float().abs().sum()) > 0
    for key, (o, n) in res.items():
        want = o0.half() if o.dtype == torch.float16 else o0
        assert torch.equal(o, want), f"output differs for {key}: max-abs {float((o.float() - want.float()).abs().max()):.3e}"
        assert torch.equal(n, n0), key
    big = torch.full((1, 256, C), 7.0e4, device=dev)
    big[:, :, 1::2] = -7.0e4
    out = torch.zeros(1, 256, C, dtype=torch.float16, device=dev)
    ops.linear(pw, x[:1, :256].contiguous(), out, B=1, H=16, W=16, dtype=dt, ldx=C, ldo=C, out_mode=ops.O_NHWC_F32, r1=big, ldr1=C)
    torch.cuda.synchronize()
    o = out.float().cpu()
    assert torch.equal(o[:, :, 0::2], torch.full_like(o[:, :, 0::2], 65504.0)) and torch.equal(o[:, :, 1::2], torch.full_like(o[:, :, 1::2], -65504.0))


@pytest.mark.parametrize("geom", [(2, 16, 40), (1, 19, 27)], ids=["B2_16x40", "ragged_19x27"])
def test_ocab_mlp_fp16_residual(geom):
    """hat_ocab_mlp with r1 as FP16 rows (out_f32 == 2, bf16 rows out for the group conv): same bits as the fp32 r1 launch."""
    from super_resolution_amd import ops
    B, H, W = geom
    dev, N, hid = _dev(), geom[1] * geom[2], 288
    w1, b1 = bf(rnd("mw1", (hid, C), std=C ** -0.5)), rnd("mb1", (hid,), std=0.2)
    w2, b2 = bf(rnd("mw2", (C, hid), std=hid ** -0.5)), rnd("mb2", (C,), std=0.2)
    pm = ops.pack_ocab_mlp(w1, b1, w2, b2, dev)
    x = bf(rnd("mx", (B, N, C))).to(torch.bfloat16).to(dev).contiguous()
    r16 = _stream("mr", B, N, dev)
    got = {}
    for half in (False, True):
        out = torch.full((B, N, C), float("nan"), dtype=torch.bfloat16, device=dev)
        ops.ocab_mlp(pm, x, r16 if half else r16.float(), out, B=B, H=H, W=W, ldx=C, ldr1=C, ldo=C, out_f32=False, dtype=ops.HAT_BF16)
        torch.cuda.synchronize()
        got[half] = out.cpu()
    assert torch.isfinite(got[False].float()).all()
    assert torch.equal(got[True], got[False])
    with pytest.raises(RuntimeError):   # FP16 r1 with an fp32 output is not a mode (out_f32 == 3)
        ops.ocab_mlp(pm, x, r16, r16.float(), B=B, H=H, W=W, ldx=C, ldr1=C, ldo=C, out_f32=True, dtype=ops.HAT_BF16)


def test_engine_hands_fp16_rows_to_proj_mlp_and_group_conv(monkeypatch):
    """On the headline configuration (HAT-S, bf16; two groups here) the OCAB projection, the OCAB MLP and the group conv must
    receive FP16 stream buffers — a silent fall-back to fp32 would pass every parity test — and HAT_NO_T16=1 must give an
    all-fp32 stream.  The two forwards round the stream at different places: they agree the way two bf16 runs do."""
    from oracle import hat_oracle as O
    from super_resolution_amd import ops
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    dev = _dev()
    kw = dict(upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01,
              overlap_ratio=0.5, img_range=1.0, depths=[2, 2], embed_dim=144, num_heads=[6, 6], mlp_ratio=2,
              upsampler="pixelshuffle", resi_connection="1conv")
    sd = synth.synth_state_dict(O.blank_state_dict(O.make_cfg(**kw)), 4321)
    x = synth.synth_input(9, (1, 3, 48, 64)).to(dev)
    seen = []
    real_conv, real_lin, real_mlp = ops.conv, ops.linear, ops.ocab_mlp

    def conv(pw, x_, out, **k):
        if k.get("r1") is not None and pw.ksize == 3 and k.get("out_mode") == ops.O_NHWC_F32:   # the group convs
            seen.append(("conv", k["r1"].dtype, out.dtype))
        return real_conv(pw, x_, out, **k)

    def linear(pw, x_, out, **k):
        if k.get("r1") is not None and k.get("ln") is not None:
            seen.append(("proj", k["r1"].dtype, out.dtype))
        return real_lin(pw, x_, out, **k)

    def mlp(pm, x_, r1, out, **k):
        seen.append(("mlp", r1.dtype, out.dtype))
        return real_mlp(pm, x_, r1, out, **k)

    monkeypatch.setattr(ops, "conv", conv)
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "ocab_mlp", mlp)

    def run():
        seen.clear()
        net = build_network(dict(type="HAT", compute_dtype="bf16", **kw)).eval()
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            y = net.to(dev)(x).float().cpu()
        torch.cuda.synchronize()
        return y, list(seen)

    y16, s16 = run()
    h = torch.float16
    assert [s for s in s16 if s[0] == "proj"] == [("proj", h, h)] * 2, s16
    assert [s for s in s16 if s[0] == "mlp"] == [("mlp", h, torch.bfloat16)] * 2, s16
    # group 0 reads the fp32 patch-embedding output and writes FP16; group 1 stays FP16 (its output is not read again)
    assert [s for s in s16 if s[0] == "conv"] == [("conv", torch.float32, h), ("conv", h, h)], s16
    monkeypatch.setenv("HAT_NO_T16", "1")
    y32, s32 = run()
    assert s32 and all(s[1] == torch.float32 and s[2] in (torch.float32, torch.bfloat16) for s in s32), s32
    assert torch.isfinite(y16).all()
    assert O.psnr_float(y16, y32) >= 44.0, O.psnr_float(y16, y32)
