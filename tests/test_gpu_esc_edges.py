"""The ESC kernels off the one shape test_gpu_esc.py runs them at, through the C ABI (super_resolution_amd.ops): hat_esc_convffn
over frames below, at and above its 8 x 12 tile and over two samples; hat_window_attention_r with q and k|v in buffers of their
own, two head counts, two samples, the smallest legal frame, the frame without reflection, the largest pad on both axes, and a
bias table shifted per head by +-100 (softmax is invariant; a kernel that mis-reduces the row maximum is not); hat_esc_layernorm
and hat_esc_shuffle_add where their grid-stride loops take several trips; the call ESCEngine.forward makes for `last`.

References are fp64 restatements (tests/esc_ref.py) on the kernels' own rounded operands, computed on the device.  Bars: fp32
max-abs 1e-4 (the ESC bar), bf16 helpers.check's; the one derived bar is stated where it is used.  Every output buffer is
pre-filled (7.0 or NaN) and its pad channels must keep the fill; pad channels of the inputs hold NaN, so reading one shows.
Every B = 2 case also asserts that sample 1 equals, bit for bit, a B = 1 launch on sample 1's rows alone.  Every case prints
the figures it is judged by."""
import math

import pytest
import torch
import torch.nn.functional as F

import esc_ref as R
from helpers import check, dev_randn, esc_ffn_sd, fill_rows, need_trips, q, rnd, run_chunked

pytestmark = pytest.mark.gpu

DT = ["f32", "bf16"]
NAN = float("nan")

# ---- outputs (pixels) the whole grid covers in ONE trip, as the launchers compute them --------------------------------------------
# hat_esc.hip hat_esc_layernorm: `const int grid = (int)(trips < 4096 ? trips : 4096);` workgroups of 16 pixels
LN64_TRIP_PIXELS = 4096 * 16
# hat_esc.hip hat_esc_shuffle_add: `dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256)`, one output value per thread
SHUF_TRIP_OUTPUTS = 8192 * 256


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def _judge(got, ref, dtype, what, f32_tol=1e-4):
    """helpers.check, after printing the figures it judges."""
    g, r = got.detach().double(), ref.detach().double().to(got.device)
    err, rel = float((g - r).abs().max()), float((g - r).norm() / max(float(r.norm()), 1e-12))
    print(f"ESC-EDGES {what} [{dtype}]: max-abs {err:.3e} rel {rel:.3e} (scale {float(r.abs().max()):.3g})")
    check(got, ref, dtype, what, f32_tol=f32_tol)


def _maps(rows, c, B, h, w):
    """(B, h*w, ld) rows -> (B, c, h, w) fp64 on the rows' device."""
    return rows[:, :, :c].double().transpose(1, 2).reshape(B, c, h, w)


def _pads_keep(rows, c, fill, what):
    assert rows.shape[2] > c and bool((rows[:, :, c:].float() == fill).all()), what + ": pad channels written"


# ------------------------------------------------------------------------------------------------
# hat_esc_convffn: shapes and batch
# ------------------------------------------------------------------------------------------------
#             1x1;  5x3: smaller than a tile, every pixel is border;  16x24: exactly 2 x 2 tiles;  9x13, B = 2: one overhanging row and column
FFN_SHAPES = [(1, 1, 1), (1, 5, 3), (1, 16, 24), (2, 9, 13)]
FFN_LD = (68, 72, 72)   # ldx, ldr, ldo


def _ffn_inputs(dtype, hid, B, H, W, dev):
    ops = _ops()
    dt = ops.DTYPE_CODE[dtype]
    sd = esc_ffn_sd(hid, dtype)
    key = f"e{hid}_{B}x{H}x{W}"
    x, r = rnd("x" + key, (B, 64, H, W)), rnd("r" + key, (B, 64, H, W))
    g, b = rnd("lng", (64,), std=0.1) + 1.0, rnd("lnb", (64,), std=0.1)
    xr = fill_rows(x.permute(0, 2, 3, 1), FFN_LD[0], torch.float32, dev, NAN)
    rr = fill_rows(r.permute(0, 2, 3, 1), FFN_LD[1], torch.float32, dev, NAN)
    return dict(pf=ops.pack_esc_convffn(sd, "f", dt, dev), sd=R.d64(sd), x=x, r=r, g=g, b=b, xr=xr, rr=rr, gd=g.to(dev), bd=b.to(dev))


def _ffn_launch(c, dtype, B, H, W, full, dev, xr=None, rr=None):
    """One hat_esc_convffn launch on rows xr / rr (default: all B samples of c) -> (out rows pre-filled with 7.0, partials or None)."""
    ops = _ops()
    dt = ops.DTYPE_CODE[dtype]
    xr, rr = c["xr"] if xr is None else xr, c["rr"] if rr is None else rr
    out = torch.full((B, H * W, FFN_LD[2]), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    parts = torch.full((B, ops.esc_convffn_tiles(H, W), 16), 7.0, device=dev) if full else None
    ops.esc_convffn(c["pf"], xr, out, B=B, H=H, W=W, dtype=dt, ln=(c["gd"], c["bd"]) if full else None, eps=R.LN_EPS,
                    r=rr if full else None, partials=parts, ldx=FFN_LD[0], ldr=FFN_LD[1], ldo=FFN_LD[2])
    torch.cuda.synchronize()
    return out, parts


def _ffn_ref(c, full):
    n = R.layernorm(c["x"].double(), c["g"].double(), c["b"].double()) if full else c["x"].double()
    return R.convffn(n, c["sd"], "f") + (c["r"].double() if full else 0.0)


def _ffn_sample1_alone(c, dtype, H, W, full, dev, out, parts):
    out1, parts1 = _ffn_launch(c, dtype, 1, H, W, full, dev, xr=c["xr"][1:2], rr=c["rr"][1:2])
    assert torch.equal(out[1:2], out1), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"
    if full:
        assert torch.equal(parts[1:2], parts1), "sample 1's pool partials differ from a B = 1 launch on its rows"


@pytest.mark.parametrize("geom", FFN_SHAPES, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("hid", [80, 128])
@pytest.mark.parametrize("dtype", DT)
def test_convffn_full_mode_shapes_and_batch(dtype, hid, geom):
    """LayerNorm + residual + pool, leading dims 68 / 72 / 72."""
    dev, ops = _dev(), _ops()
    B, H, W = geom
    c = _ffn_inputs(dtype, hid, B, H, W, dev)
    out, parts = _ffn_launch(c, dtype, B, H, W, True, dev)
    got = _maps(out, 64, B, H, W)
    _judge(got, _ffn_ref(c, True), dtype, f"hat_esc_convffn hid {hid} {B}x{H}x{W}")
    _pads_keep(out, 64, 7.0, "hat_esc_convffn out")
    # the pool partials: one slot per sample and tile, the sums of the stored values of channels 0..15 over the tile's pixels
    tiles = -(-H // 8) * -(-W // 12)
    assert ops.esc_convffn_tiles(H, W) == tiles and parts.shape == (B, tiles, 16)
    want = torch.stack([torch.stack([got[b, :16, ty:ty + 8, tx:tx + 12].sum((1, 2)) for ty in range(0, H, 8) for tx in range(0, W, 12)])
                        for b in range(B)])
    err = float((parts.double() - want).abs().max())
    print(f"ESC-EDGES convffn pool partials {B}x{H}x{W} [{dtype}]: max-abs {err:.3e} (scale {float(want.abs().max()):.3g})")
    assert err <= 1e-4 * max(1.0, float(want.abs().max())), err
    out2, parts2 = _ffn_launch(c, dtype, B, H, W, True, dev)
    assert torch.equal(out, out2) and torch.equal(parts, parts2), "two runs differ"
    if B == 2:
        assert not torch.equal(out[0], out[1])
        _ffn_sample1_alone(c, dtype, H, W, True, dev, out, parts)


@pytest.mark.parametrize("hid", [80, 128])
@pytest.mark.parametrize("dtype", DT)
def test_convffn_plain_mode_two_samples(dtype, hid):
    """No LayerNorm, no residual, no pool, B = 2 on 9 x 13."""
    dev = _dev()
    B, H, W = 2, 9, 13
    c = _ffn_inputs(dtype, hid, B, H, W, dev)
    out, _ = _ffn_launch(c, dtype, B, H, W, False, dev)
    _judge(_maps(out, 64, B, H, W), _ffn_ref(c, False), dtype, f"hat_esc_convffn plain hid {hid} {B}x{H}x{W}")
    _pads_keep(out, 64, 7.0, "hat_esc_convffn out")
    _ffn_sample1_alone(c, dtype, H, W, False, dev, out, None)


# ------------------------------------------------------------------------------------------------
# hat_window_attention_r: q and k|v in buffers of their own, heads, batch, frames, stiff softmax
# ------------------------------------------------------------------------------------------------
def _attn_inputs(dtype, heads, B, h, w, dev, shift=None):
    """q in its own buffer (ldq 72), k|v in another (ldkv 2C + 8); -> rows, the table as stored (fp32, device) and the reflect-padded
    fp64 qkv maps (B, 3C, Hp, Wp) on the device, q NOT yet scaled (attention_core divides by sqrt(d))."""
    ops = _ops()
    tdt = ops.TORCH_DTYPE[ops.DTYPE_CODE[dtype]]
    C = 16 * heads
    key = f"wa{heads}_{B}x{h}x{w}"
    qm, km, vm = (q(rnd(n + key, (B, C, h, w)), dtype) for n in "qkv")
    table = rnd("rpb32e", (heads, 63 * 63), std=0.5)
    if shift is not None:
        table = table + torch.tensor(shift, dtype=torch.float32)[:, None]     # fp32, as stored: the reference reads this table
    ldq, ldkv, ldo = 72, 2 * C + 8, C + 8
    qr = fill_rows(qm.permute(0, 2, 3, 1) * 0.25, ldq, tdt, dev, NAN)         # pre-multiplied by head_dim^-0.5: a power of two, exact
    kvr = fill_rows(torch.cat([km, vm], 1).permute(0, 2, 3, 1), ldkv, tdt, dev, NAN)
    padded = R.reflect_pad(torch.cat([qm, km, vm], 1).double().to(dev), 32)
    return dict(C=C, heads=heads, qr=qr, kvr=kvr, table=table.to(dev), padded=padded, ld=(ldq, ldkv, ldo), vmax=float(vm.abs().max()))


def _attn_launch(c, dtype, B, h, w, dev, qr=None, kvr=None):
    ops = _ops()
    dt = ops.DTYPE_CODE[dtype]
    ldq, ldkv, ldo = c["ld"]
    out = torch.full((B, h * w, ldo), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.window_attention_r(c["qr"] if qr is None else qr, c["kvr"] if kvr is None else kvr, c["table"], out, B=B, h=h, w=w, C_=c["C"],
                           heads=c["heads"], ws=32, ldq=ldq, ldkv=ldkv, ldo=ldo, dtype=dt)
    torch.cuda.synchronize()
    return out


#              17x17, B = 2: the smallest legal frame, both pads 15, one window;  32x32: no reflection;  33x65: pad 31 on both axes, 2 x 3 windows
ATTN_CASES = [(2, 2, 17, 17), (4, 2, 17, 17), (4, 1, 32, 32), (4, 1, 33, 65), (2, 1, 33, 65)]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"heads{c[0]}_{c[1]}x{c[2]}x{c[3]}")
@pytest.mark.parametrize("dtype", DT)
def test_window_attention_r_split_buffers_heads_batch_frames(dtype, case):
    dev = _dev()
    heads, B, h, w = case
    c = _attn_inputs(dtype, heads, B, h, w, dev)
    out = _attn_launch(c, dtype, B, h, w, dev)
    ref = R.attention_core(c["padded"], c["table"].double(), 32, heads)[:, :, :h, :w]
    _judge(_maps(out, c["C"], B, h, w), ref, dtype, f"hat_window_attention_r heads {heads} {B}x{h}x{w}")
    _pads_keep(out, c["C"], 7.0, "hat_window_attention_r out")
    if B == 2:
        assert not torch.equal(out[0], out[1])
        out1 = _attn_launch(c, dtype, 1, h, w, dev, qr=c["qr"][1:2], kvr=c["kvr"][1:2])
        assert torch.equal(out[1:2], out1), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


def _ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23)


@pytest.mark.parametrize("dtype", DT)
def test_window_attention_r_is_invariant_to_a_per_head_bias_shift(dtype):
    """The bias table of heads 0..3 shifted by +100, -100, 0, +30: softmax does not change, but without the row maximum head 0
    overflows exp and head 1 divides by zero.  The reference is fp64 on the fp32 table as stored.  fp32 bar, this case only:
    1e-4 + 8 ulp32(max |logit|) * 2 max |v|: a logit near 100 carries about 7.6e-6 of fp32 rounding, which softmax passes to the
    output at most twice over (an error eps on the logits moves a softmax-weighted mean of v by at most 2 eps max |v|)."""
    dev = _dev()
    heads, B, h, w = 4, 1, 17, 17
    c = _attn_inputs(dtype, heads, B, h, w, dev, shift=[100.0, -100.0, 0.0, 30.0])
    ref, logit = R.attention_core(c["padded"], c["table"].double(), 32, heads, logits=True)
    ref = ref[:, :, :h, :w]
    top = [float(logit[:, i].max()) for i in range(heads)]
    assert top[0] > 89.0 and top[1] < -89.0, top      # exp(89) overflows fp32, exp(-89) is below its normal range
    out = _attn_launch(c, dtype, B, h, w, dev)
    got = _maps(out, 64, B, h, w)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = float((got - ref).abs().max())
    bar = 1e-4 + 8 * _ulp32(float(logit.abs().max())) * 2 * c["vmax"]
    print(f"ESC-EDGES hat_window_attention_r shifted bias [{dtype}]: max-abs {err:.3e}, fp32 bar {bar:.3e} "
          f"(max |logit| {float(logit.abs().max()):.2f}, max |v| {c['vmax']:.3f}, top logits per head {[round(t, 2) for t in top]})")
    if dtype == "f32":
        assert err <= bar, f"max-abs {err:.3e} > {bar:.3e}"
    else:
        check(got, ref, dtype, "hat_window_attention_r shifted bias")
    _pads_keep(out, 64, 7.0, "hat_window_attention_r out")


def test_window_attention_r_refuses_bad_layouts():
    dev, ops = _dev(), _ops()
    C = 64
    qr, kvr = torch.zeros(1, 40 * 40, 72, device=dev), torch.zeros(1, 40 * 40, 2 * C + 8, device=dev)
    o, t = torch.zeros(1, 40 * 40, C + 8, device=dev), torch.zeros(4, 63 * 63, device=dev)
    kw = dict(B=1, h=40, w=40, C_=C, heads=4, ws=32, ldq=72, ldkv=2 * C + 8, ldo=C + 8, dtype=ops.HAT_F32)
    ops.window_attention_r(qr, kvr, t, o, **kw)                                     # the layout itself is accepted
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.window_attention_r(qr, kvr, t, o, **dict(kw, ldkv=2 * C - 4))           # v would run into the next row
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.window_attention_r(qr, kvr, t, o, **dict(kw, ldq=70))                   # fp32 rows are read 4 floats at a time
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.window_attention_r(qr.bfloat16(), kvr.bfloat16(), t, o.bfloat16(), **dict(kw, ldq=68, dtype=ops.HAT_BF16))   # bf16: 8 at a time
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.window_attention_r(qr, kvr.view(-1)[1:], t, o, **kw)                    # a kv pointer 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.window_attention_r(qr, kvr, t, o, **dict(kw, heads=3))                  # C != 16 heads
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.window_attention_r(qr, kvr, t, o, **dict(kw, h=40, w=16))               # 16 columns cannot be reflect-padded to 32
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# hat_esc_layernorm and hat_esc_shuffle_add: several trips of the grid-stride loops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_esc_layernorm_multitrip(dtype):
    """3 x 65536 + 16 x 1000 + 5 pixels: 1000 workgroups take 4 trips, the others 3, the last tile holds 5 pixels."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    npix, ldx, ldy, spare = 3 * 65536 + 16 * 1000 + 5, 68, 72, 16
    need_trips(npix, LN64_TRIP_PIXELS, 4, "hat_esc_layernorm")
    x = torch.full((1, npix + spare, ldx), NAN, device=dev)
    x[:, :npix, :64] = dev_randn("ln64x", (1, npix, 64), dev, std=1.5, mean=0.3)
    g, b = (1 + rnd("ln64g", (64,), std=0.1)).to(dev), rnd("ln64b", (64,), std=0.1).to(dev)

    def launch(xv, yv):
        ops.esc_layernorm(xv, yv, g, b, npix=xv.shape[1], dtype=dt, eps=1e-6, ldx=ldx, ldy=ldy)

    y = torch.full((1, npix + spare, ldy), NAN, dtype=tdt, device=dev)
    launch(x[:, :npix], y[:, :npix])                          # LN64_TRIP_PIXELS per trip
    torch.cuda.synchronize()
    ref = F.layer_norm(x[:, :npix, :64].double(), (64,), g.double(), b.double(), 1e-6)
    _judge(y[:, :npix, :64].float(), ref, dtype, "hat_esc_layernorm 212613 px")
    assert bool(torch.isnan(y[:, :npix, 64:].float()).all()), "pad channels written"
    assert bool(torch.isnan(y[:, npix:].float()).all()), "rows past npix written"
    y2 = torch.full_like(y, NAN)
    run_chunked(lambda v, _b: launch(v["x"], v["y"]), dict(x=x[:, :npix], y=y2[:, :npix]), 1, npix, LN64_TRIP_PIXELS)
    torch.cuda.synchronize()
    assert torch.equal(y[:, :npix, :64], y2[:, :npix, :64]), "the multi-trip launch differs from its one-trip chunks"


def test_esc_layernorm_bf16_rows_35_pixels():
    """The bf16 store at kernel level, beside test_gpu_esc.py's fp32 case: small rows, so eps 1e-6 against 1e-5 is visible."""
    dev, ops = _dev(), _ops()
    x = rnd("lnx", (1, 64, 5, 7), std=1e-3)
    g, b = rnd("lng", (64,), std=0.1) + 1.0, rnd("lnb", (64,), std=0.1)
    xr = fill_rows(x.permute(0, 2, 3, 1), 68, torch.float32, dev, NAN)
    y = torch.full((1, 35, 72), 7.0, dtype=torch.bfloat16, device=dev)
    ops.esc_layernorm(xr, y, g.to(dev), b.to(dev), npix=35, dtype=ops.HAT_BF16, eps=1e-6, ldx=68, ldy=72)
    torch.cuda.synchronize()
    ref = R.layernorm(x.double(), g.double(), b.double(), 1e-6)
    _judge(_maps(y, 64, 1, 5, 7), ref, "bf16", "hat_esc_layernorm 35 px")
    _pads_keep(y, 64, 7.0, "hat_esc_layernorm y")
    with pytest.raises(AssertionError):      # the bf16 bars can tell the two eps apart
        check(_maps(y, 64, 1, 5, 7), R.layernorm(x.double(), g.double(), b.double(), 1e-5), "bf16", "eps 1e-5")


def _shuffle_case(s, B, H, W, ld, dev, rows, img):
    """rows (B, H*W, ld) with NaN pad channels, img (B,3,H,W), both on the device -> asserts bit equality with the plain expression."""
    ops = _ops()
    n = 3 * s * s
    out = torch.full((B, 3, H * s, W * s), NAN, device=dev)
    ops.esc_shuffle_add(rows, img, out, B=B, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    want = F.pixel_shuffle(rows[:, :, :n].reshape(B, H, W, n).permute(0, 3, 1, 2) + torch.repeat_interleave(img, s * s, dim=1), s)
    assert torch.equal(out, want), f"hat_esc_shuffle_add x{s} {B}x{H}x{W}"
    return out


def test_esc_shuffle_add_multitrip():
    """x3, B = 2, 331 x 301, ld 28: 5.38 M outputs, so threads take 3 and 2 trips, and sample 1 starts inside a trip."""
    dev = _dev()
    s, B, H, W, ld = 3, 2, 331, 301, 28
    need_trips(B * 3 * H * s * W * s, SHUF_TRIP_OUTPUTS, 3, "hat_esc_shuffle_add")
    rows = torch.full((B, H * W, ld), NAN, device=dev)
    rows[:, :, :27] = dev_randn("shufrows", (B, H * W, 27), dev)
    img = dev_randn("shufimg", (B, 3, H, W), dev)
    out = _shuffle_case(s, B, H, W, ld, dev, rows, img)     # SHUF_TRIP_OUTPUTS per trip
    out1 = torch.full((1, 3, H * s, W * s), NAN, device=dev)
    _ops().esc_shuffle_add(rows[1:2], img[1:2], out1, B=1, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    assert torch.equal(out[1:2], out1), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


@pytest.mark.parametrize("s", [2, 4])
def test_esc_shuffle_add_two_samples(s):
    dev = _dev()
    B, H, W, ld = 2, 5, 7, 3 * s * s + 4
    rows = fill_rows(rnd(f"sh2_{s}", (B, H, W, 3 * s * s)), ld, torch.float32, dev, NAN)
    img = rnd(f"sh2x{s}", (B, 3, H, W)).to(dev)
    out = _shuffle_case(s, B, H, W, ld, dev, rows, img)
    out1 = torch.full((1, 3, H * s, W * s), NAN, device=dev)
    _ops().esc_shuffle_add(rows[1:2], img[1:2], out1, B=1, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    assert torch.equal(out[1:2], out1) and not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------
# hat_conv as ESCEngine.forward calls it for `last`
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_conv_last_from_f32_rows_with_residual_to_T_rows(dtype):
    """3x3 64 -> 64 read from the fp32 stream (x_mode X_NHWC_F32), + feat0 (r1, fp32 rows), stored as T rows for to_img."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    B, H, W, C = 1, 20, 37, 64
    x, r1 = rnd("lastx", (B, H, W, C)), rnd("lastr", (B, H, W, C))
    wgt, bias = q(rnd("lastw", (C, C, 3, 3), std=(9 * C) ** -0.5), dtype), rnd("lastb", (C,), std=0.1)
    pw = ops.pack_conv_weight(wgt, bias, dt, dev)
    xd, rd = x.reshape(B, H * W, C).to(dev).contiguous(), r1.reshape(B, H * W, C).to(dev).contiguous()
    out = torch.full((B, H * W, C), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.conv(pw, xd, out, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, x_mode=ops.X_NHWC_F32, r1=rd, ldr1=C)
    torch.cuda.synchronize()
    ref = F.conv2d(q(x, dtype).permute(0, 3, 1, 2).double(), wgt.double(), bias.double(), padding=1) + r1.permute(0, 3, 1, 2).double()
    _judge(_maps(out, C, B, H, W), ref.to(dev), dtype, "hat_conv last 64 -> 64 from fp32 rows + r1")
    assert torch.equal(xd.cpu(), x.reshape(B, H * W, C)) and torch.equal(rd.cpu(), r1.reshape(B, H * W, C)), "an operand was written"
