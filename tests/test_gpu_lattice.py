"""Exact-lattice parity of the linear MFMA kernels (tests/lattice.py; DESIGN "Exact-lattice parity tests"), THROUGH THE C ABI: with
every operand on a small dyadic lattice the fp64 reference is the only answer a kernel may give — fp32 outputs bit-equal to it,
bf16 / FP16 outputs equal to its one round-to-nearest-even — so a wrong tap, halo, pad-channel read, border rule, bias or residual
at any single pixel is a failing element.  Input pad channels hold a poison value, outputs are pre-filled: channels past n_store
keep the fill.  Behind a pointwise activation the exact sum S is known and the kernel may be one ulp of the output type off
act(S).  test_lattice_cpu.py checks every case's domain condition and that the method catches what helpers.check lets through."""
import pytest
import torch
import torch.nn.functional as F

import lattice as L
from helpers import _r8, check, fill_rows, rnd

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def _rows(x_bhwc, ld, tdt, dev, c_zero=None):
    """helpers.fill_rows with the poison value (lattice values are exact in fp32, so the fp64 operands pass through it unchanged)."""
    return fill_rows(x_bhwc.to(torch.float32), ld, tdt, dev, L.POISON, c_zero=c_zero)


def _run(c: L.Case, kind: str):
    """Launch one lattice.conv_case on hat_conv ("conv"), hat_linear ("linear") or hat_conv3x3_small ("t3") and hold it to the
    reference.  Without an activation the expectation is the reference rounded once (lattice.expect).  Behind one, act(S) is no
    fp32 number: it goes fp64 -> fp32 -> T (torch has no fp64 -> bf16 conversion), two roundings that can differ from the single
    one by an ulp of T only at a tie the first one created; the one-ulp rule is applied to that value and not widened for it."""
    dev, ops = _dev(), _ops()
    from super_resolution_amd import packing
    o, (B, H, W), cin, cout, k = c.opt, c.geom, c.cin, c.cout, c.k
    dt = ops.DTYPE_CODE[c.dtype]
    tdt = ops.TORCH_DTYPE[dt]
    what = f"{kind} k{k} {cin}->{cout} {c.geom} {c.dtype} {o}"
    # weights
    wt, bs = c.w.to(torch.float32), c.bias.to(torch.float32)
    if kind == "conv":
        pw = ops.pack_conv_weight(wt, bs, dt, dev, out_perm=packing.pixshuf_perm(cout, o["ps_r"]) if o["out"] == "ps" else None)
    else:
        pw = ops.pack_linear_weight(wt if k > 1 else wt.reshape(cout, cin), bs, dt, dev)
    kw = dict(B=B, H=H, W=W, dtype=dt, act=o["act"])
    # input
    if o["x"] == "nchw_mean":
        xd, kw["ldx"] = c.x_src.to(torch.float32).to(dev).contiguous(), 0
        kw.update(x_mode=ops.X_NCHW_F32_MEAN, in_scale=c.in_scale, mean=c.mean)
    elif o["x"] == "f32":
        kw["ldx"] = cin + 4
        xd = _rows(c.x, kw["ldx"], torch.float32, dev)
        kw["x_mode"] = ops.X_NHWC_F32
    else:
        kw["ldx"] = _r8(cin) + 8
        xd = _rows(c.x, kw["ldx"], tdt, dev, c_zero=_r8(cin))
    if o["c_split"]:
        kw.update(x0=_rows(c.x0, o["c_split"] + 8, tdt, dev), c_split=o["c_split"], ldx0=o["c_split"] + 8)
    # residuals
    r1d = None
    if o["r1"] in ("f32", "f16"):
        r1t = torch.float16 if o["r1"] == "f16" else torch.float32
        r1d = _rows(c.r1, cout + 8, r1t, dev)
        kw.update(r1=r1d, ldr1=cout + 8)
    if o["r2"]:
        sc = torch.zeros(B, pw.npad, device=dev)
        sc[:, :cout] = c.r2scale.to(torch.float32).to(dev)
        kw.update(r2=_rows(c.r2, cout + 8, tdt, dev), ldr2=cout + 8, r2scale=sc, r2scale_bstride=pw.npad)
    # output
    n_store = (cout + 3) // 4 * 4
    if o["out"] == "T":
        odt, ldo = tdt, _r8(cout) + 8
        out = torch.full((B, H * W, ldo), L.FILL, dtype=odt, device=dev)
        kw["n_store"] = n_store
    elif o["out"] in ("f32", "f16"):
        odt, ldo = (torch.float32 if o["out"] == "f32" else torch.float16), cout + 8
        out = _rows(c.r1, ldo, odt, dev) if o["r1"] == "inplace" else torch.full((B, H * W, ldo), L.FILL, dtype=odt, device=dev)
        if o["r1"] == "inplace":
            out[:, :, cout:] = L.FILL
            kw.update(r1=out, ldr1=ldo)
        kw["out_mode"] = ops.O_NHWC_F32
    elif o["out"] == "ps":
        r = o["ps_r"]
        odt, ldo = tdt, cout // (r * r) + 8
        out = torch.full((B, H * r * W * r, ldo), L.FILL, dtype=odt, device=dev)
        kw.update(out_mode=ops.O_PIXSHUF_T, ps_r=r)
    else:
        odt, ldo = torch.float32, 0
        out = torch.full((B, cout, H, W), L.FILL, dtype=odt, device=dev)
        kw.update(out_mode=ops.O_NCHW_F32, out_scale=c.out_scale, mean=c.mean, n_store=cout)
    kw["ldo"] = ldo
    colsum = None
    if o["colsum"]:
        parts = ops.conv_tiles(pw, H, W, dt) if kind == "conv" else ops.conv3x3_small_groups(pw, B, H, W, dt)
        colsum = torch.full((B, parts, pw.npad), L.FILL, dtype=torch.float32, device=dev)
        kw["colsum"] = colsum
    if o["ln"]:
        g, bt = 1.0 + rnd("lat.lg", (cout,), std=0.2), rnd("lat.lb", (cout,), std=0.2)
        ln_out = torch.full((B, H * W, cout), L.FILL, dtype=tdt, device=dev)
        n16 = torch.full((B, H * W, 16), L.FILL, dtype=tdt, device=dev)
        gap = torch.full((B, ops.conv_tiles(pw, H, W, dt), 16), L.FILL, dtype=torch.float32, device=dev)
        kw.update(ln=(g.to(dev), bt.to(dev)), ln_out=ln_out, ld_ln=cout, gap_out=gap, gap_c=16, n16_out=n16)
    if kind == "linear":
        assert ops.linear_supported(cout, cin, dt)
        ops.linear(pw, xd, out, **kw)
    elif kind == "t3":
        assert ops.conv3x3_small_supported(cout, cin, dt)
        ops.conv3x3_small(pw, xd, out, **kw)
    else:
        ops.conv(pw, xd, out, **kw)
    torch.cuda.synchronize()
    # the expectation: the reference rounded once; behind an activation act(S), through fp32, within one ulp
    if o["out"] == "ps":
        ref = L.pixel_shuffle_last(c.ref, o["ps_r"])
        got = out[:, :, :ref.shape[-1]].reshape(ref.shape)
    elif o["out"] == "nchw":
        ref, got = c.ref.permute(0, 3, 1, 2).contiguous(), out
    else:
        ref, got = c.ref, out[:, :, :cout].reshape(B, H, W, cout)
    if o["act"]:
        want = L.act64(ref, o["act"]).to(torch.float32).to(odt)
        L.assert_ulp(got, want, what)
    else:
        want = L.expect(ref, odt)
        L.assert_bits(got, want, what)
    if o["out"] == "T":
        assert torch.all(out[:, :, cout:n_store] == 0), what + ": channels between Cout and n_store are zeros"
        assert torch.all(out[:, :, n_store:] == L.FILL), what + ": channels past n_store keep the fill"
    elif o["out"] != "nchw":
        assert torch.all(out[:, :, got.shape[-1]:] == L.FILL), what + ": pad channels of the output keep the fill"
    if r1d is not None:
        assert torch.equal(r1d[:, :, :cout].cpu().double(), c.r1.reshape(B, H * W, cout)), what + ": r1 is only read"
    if colsum is not None:
        tot = colsum.double().sum(1).cpu()
        assert torch.all(tot[:, cout:] == 0), what + ": column sums of the pad channels"
        if o["act"]:     # sums of the STORED values, which are off the lattice: fp32 round-off of the summation only
            check(tot[:, :cout] / (H * W), got.double().cpu().sum((1, 2)) / (H * W), "f32", what + " column sums of the stored values")
        else:            # integer sums of the stored (once-rounded) values: exact
            stored = want.double().sum((1, 2))
            assert torch.equal(tot[:, :cout], stored), f"{what}: column sums differ by up to {float((tot[:, :cout] - stored).abs().max())}"
    if o["ln"]:
        check(ln_out.float().reshape(B, H, W, cout), F.layer_norm(c.ref, (cout,), g.double(), bt.double(), 1e-5), c.dtype, what + " fused LayerNorm",
              f32_tol=6e-5)
        assert torch.equal(n16, ln_out[:, :, :16]), what + ": compact 16-channel copy"
    return out


# ------------------------------------------------------------------------------------------------
# hat_conv (and hat_conv64r behind it)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("geom", L.GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("shape", L.CONV_PLAIN, ids=lambda s: f"k{s[0]}_{s[1]}to{s[2]}")
def test_conv_plain_is_exact(shape, geom, dtype):
    k, cin, cout = shape
    _run(L.conv_case(f"conv{k}.{cin}.{cout}.{geom}", geom, k, cin, cout, dtype), "conv")


_FORMS = [(f, d) for f in L.CONV_FORMS for d in f.dtypes]


@pytest.mark.parametrize("form,dtype", _FORMS, ids=[f"{f.name}-{d}" for f, d in _FORMS])
def test_conv_forms_are_exact(form, dtype):
    """Every linear epilogue, input and output form of hat_conv: fp32 / in-place / FP16-row residuals, the scaled T residual, the
    split source, the NCHW first conv, fp32 token rows in, pixel shuffle at r = 2, 3 on the resident-weight kernel and beside it,
    fp32 rows and NCHW planes out, FP16 residual-stream rows, column sums, the fused LayerNorm's main output and n16 copy; GELU and
    LeakyReLU within one ulp of act(S)."""
    _run(L.conv_case("form." + form.name, form.geom, form.k, form.cin, form.cout, dtype, form.opt), "conv")


# ------------------------------------------------------------------------------------------------
# hat_linear: every instantiated (nt, ceil(Cin / 32))
# ------------------------------------------------------------------------------------------------
_LIN = [(s, g, f, d) for s in L.LIN_SHAPES for g in L.LIN_GEOMS for f in L.LIN_FORMS for d in L.lin_dtypes(s[1], s[2]) if f != "gelu" or d == "bf16"]


@pytest.mark.parametrize("shape,geom,form,dtype", _LIN, ids=[f"{s[0]}-{'x'.join(map(str, g))}-{f}-{d}" for s, g, f, d in _LIN])
def test_linear_is_exact(shape, geom, form, dtype):
    name, cin, cout = shape
    _run(L.conv_case(f"lin.{name}.{geom}.{form}", geom, 1, cin, cout, dtype, L.LIN_FORMS[form]), "linear")


@pytest.mark.parametrize("form", list(L.LIN_FP16))
def test_linear_fp16_residual_rows_are_exact(form):
    """The OCAB-projection form: FP16 r1 and / or FP16 output rows (one rounding to FP16 of the exact sum)."""
    _run(L.conv_case(f"lin.aggr144.{form}", (2, 19, 27), 1, 144, 144, "bf16", L.LIN_FP16[form]), "linear")


# ------------------------------------------------------------------------------------------------
# hat_conv3x3_small: the four instantiations, with column sums
# ------------------------------------------------------------------------------------------------
_T3 = [(s, a, d) for s in L.T3_SHAPES for a in (0, 1, 2) for d in L.t3_dtypes(s[1], s[2]) if a != 1 or d == "bf16"]


@pytest.mark.parametrize("shape,act,dtype", _T3, ids=[f"{s[0]}-act{a}-{d}" for s, a, d in _T3])
def test_conv3x3_small_is_exact(shape, act, dtype):
    name, cin, cout = shape
    _run(L.conv_case(f"t3.{name}.{act}", L.T3_GEOM, 3, cin, cout, dtype, dict(colsum=True, act=act)), "t3")


# ------------------------------------------------------------------------------------------------
# hat_aggr_cab
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", L.AGGR_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_aggr_cab_is_exact(geom):
    dev, ops = _dev(), _ops()
    from super_resolution_amd import packing
    c = L.aggr_case(geom)
    B, H, W = geom
    C, bf = c.C, torch.bfloat16
    pw = ops.pack_linear_weight(c.wa.float(), None, ops.HAT_BF16, dev)
    wf = torch.stack([packing.pack_cab_w2f(c.wf[b].float(), "cpu").reshape(-1) for b in range(B)]).to(bf).to(dev).contiguous()
    assert wf.shape == (B, pw.nt * 3 * 512)
    bias_b = torch.zeros(B, pw.npad, device=dev)
    bias_b[:, :C] = c.bias_b.float().to(dev)
    ld = C + 8
    r1 = _rows(c.r1, ld, torch.float32, dev)
    for inplace in (False, True):
        out = r1.clone() if inplace else torch.full((B, H * W, ld), L.FILL, device=dev)
        out[:, :, C:] = L.FILL
        ops.aggr_cab(pw, _rows(c.x, ld, bf, dev), out, _rows(c.c1, 8, bf, dev), wf, bias_b, B=B, H=H, W=W, dtype=ops.HAT_BF16, ldx=ld, ldo=ld,
                     x0=_rows(c.x0, 24, bf, dev), c_split=16, ldx0=24, r1=(out if inplace else r1), ldr1=ld)
        torch.cuda.synchronize()
        L.assert_bits(out[:, :, :C].reshape(B, H, W, C), L.expect(c.ref, torch.float32), f"aggr + folded cab {geom} inplace={inplace}")
        assert torch.all(out[:, :, C:] == L.FILL)


# ------------------------------------------------------------------------------------------------
# hat_esc_conv13, and hat_conv k = 13 on the same operands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", L.ESC13_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_esc_conv13_is_exact_and_equals_hat_conv(geom):
    dev, ops = _dev(), _ops()
    c = L.esc13_case(geom)
    B, H, W = geom
    dt, bf, pd, ks = ops.HAT_BF16, torch.bfloat16, 16, 13
    kc = ops.KC[dt] * 3
    kpad = -(-(ks * ks * pd) // kc) * kc
    wp = torch.zeros(B, 16, kpad)
    wp[:, :, :ks * ks * pd] = c.w.float().permute(0, 1, 3, 4, 2).reshape(B, pd, ks * ks * pd)      # K = tap * 16 + ci
    wpd = wp.to(bf).to(dev).contiguous()
    xd = _rows(c.x, 144, bf, dev)                     # channels 16.. of the 144-wide rows: nothing may read them
    want = L.expect(c.ref, bf)
    y = torch.full((B, H * W, 16), L.FILL, dtype=bf, device=dev)
    ops.esc_conv13(xd, wpd, y, B=B, H=H, W=W, ldx=144, kpad=kpad, dtype=dt)
    torch.cuda.synchronize()
    L.assert_bits(y.reshape(B, H, W, 16), want, f"esc conv13 {geom}")
    pw = ops.PackedConv(wpd, torch.zeros(16, device=dev), ks, pd, kpad, 1, 1, pd, w_bstride=16 * kpad)
    y2 = torch.full_like(y, L.FILL)
    ops.conv(pw, xd, y2, B=B, H=H, W=W, dtype=dt, ldx=144, ldo=16, n_store=16)
    torch.cuda.synchronize()
    L.assert_bits(y2.reshape(B, H, W, 16), want, f"hat_conv k13 with per-sample weights {geom}")
    assert torch.equal(y, y2)


# ------------------------------------------------------------------------------------------------
# the row-sweep 3 x 3 kernel: hat_conv3x3_to_planes (exact) and hat_cab_squeeze (GELU of the exact sum)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", L.SWEEP_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_conv3x3_to_planes_is_exact(geom):
    dev, ops = _dev(), _ops()
    B, H, W = geom
    for nout in (3, 1):
        c = L.sweep_case(geom, 64, nout, gelu=False)
        wpk, b8 = ops.pack_cab_squeeze(c.w.float(), c.bias.float(), dev)
        out = torch.full((B, nout, H, W), L.FILL, device=dev)
        ops.conv3x3_to_planes(_rows(c.x, 72, torch.bfloat16, dev).reshape(B, H, W, 72), wpk, b8, out, B=B, H=H, W=W, C_=64, ldx=72, n_out=nout,
                              out_scale=c.out_scale, mean=c.mean, dtype=ops.HAT_BF16)
        torch.cuda.synchronize()
        L.assert_bits(out.permute(0, 2, 3, 1), L.expect(c.ref, torch.float32), f"conv_last planes {geom} n_out={nout}")


_SQ = [(g, cm) for g in L.SWEEP_GEOMS for cm in L.SQUEEZE_CM]


@pytest.mark.parametrize("geom,cm", _SQ, ids=[f"{'x'.join(map(str, g))}-C{cm[0]}_mid{cm[1]}" for g, cm in _SQ])
def test_cab_squeeze_is_gelu_of_the_exact_sum(geom, cm):
    """hat_cab_squeeze always ends in GELU: the stored value is within one bf16 ulp of GELU(S), S the exact sum (|S| <= 4).  Its
    column sums add stored values, which are off the lattice: against their fp64 sum on helpers.check's fp32 bar."""
    dev, ops = _dev(), _ops()
    B, H, W = geom
    C, mid = cm
    c = L.sweep_case(geom, C, mid, gelu=True)
    wpk, b8 = ops.pack_cab_squeeze(c.w.float(), c.bias.float(), dev)
    units = ops.cab_squeeze_units(H, W)
    out = torch.full((B, H, W, 8), L.FILL, dtype=torch.bfloat16, device=dev)
    cs = torch.full((B, units, 16), L.FILL, dtype=torch.float32, device=dev)
    ld = C + 8
    ops.cab_squeeze(_rows(c.x, ld, torch.bfloat16, dev).reshape(B, H, W, ld), wpk, b8, out, cs, B=B, H=H, W=W, C_=C, ldx=ld, dtype=ops.HAT_BF16)
    torch.cuda.synchronize()
    L.assert_ulp(out[..., :mid], L.act64(c.ref, 1).to(torch.float32).to(torch.bfloat16), f"cab squeeze {geom} C={C} mid={mid}")
    assert torch.all(out[..., mid:] == 0), "channels past mid are zeros"
    tot = cs.double().sum(1).cpu()
    assert torch.all(tot[:, 8:] == 0)
    check(tot[:, :mid] / (H * W), out[..., :mid].double().cpu().sum((1, 2)) / (H * W), "f32", "column sums of the stored values")


# ------------------------------------------------------------------------------------------------
# hat_upfold_to_planes against the three operations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", L.UPFOLD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upfold_is_exact_against_the_three_operations(shape):
    """Bit for bit against conv -> pixel_shuffle -> conv in fp64 (not packing.upfold_apply: the packer's border variants are under
    test), on the four corners, on the border ring and everywhere."""
    dev, ops = _dev(), _ops()
    H, W = shape
    c = L.upfold_case(shape)
    B = c.geom[0]
    out = torch.full((B, 3, 2 * H, 2 * W), L.FILL, device=dev)
    ops.upfold_to_planes(_rows(c.x, 72, torch.bfloat16, dev), ops.pack_upfold(*(t.float() for t in c.w), dev), out, B=B, H=H, W=W, ldx=72,
                         out_scale=c.out_scale, mean=c.mean, dtype=ops.HAT_BF16)
    torch.cuda.synchronize()
    got, want = out.cpu().permute(0, 2, 3, 1), L.expect(c.ref, torch.float32).permute(0, 2, 3, 1)
    ys, xs = [0, 1, 2 * H - 2, 2 * H - 1], [0, 1, 2 * W - 2, 2 * W - 1]
    L.assert_bits(got[:, ys][:, :, xs], want[:, ys][:, :, xs], f"upfold {shape}: the 2 x 2 outputs of the four corner pixels")
    ring = L.ring_mask(2 * H, 2 * W)
    ring[:2], ring[-2:], ring[:, :2], ring[:, -2:] = True, True, True, True
    L.assert_bits(got[:, ring], want[:, ring], f"upfold {shape}: the outputs of the border ring")
    L.assert_bits(got, want, f"upfold {shape}")
