"""The ESCReal, ESCRealM, ESCFP and ESC-LTE kernels off the shapes their own tests run them at, through the C ABI
(super_resolution_amd.ops): hat_unshuffle_pad, hat_shuffle_planes, hat_escfp_shuffle_bicubic and hat_dysample where their
grid-stride loops take three trips and a sample starts inside a trip; B = 2 on the five entries whose contract offers it;
hat_escreal_skip at exactly one 64-pixel tile and on frames narrower than its 7-tap window; hat_escrealm_skip where an 8 x 8 tile
overhangs by one pixel (the clamp of the dropped pixels' halo), at the minimum height and at exact tile multiples; hat_lte_query
with the affine in explicit mode, coef and freq in buffers of their own, one-pixel and one-column maps, and a grid smaller than
the map.

References are fp64 restatements (tests/escreal_ref.py, escrealm_ref.py, esclte_ref.py) on the kernels' own rounded operands,
computed on the device where the frame is large.  Bars: fp32 max-abs 1e-4 (the ESC family's), bf16 helpers.check's, exact equality
for the data movers, test_shuffle_bicubic_matches_torch's 1e-4 for the bicubic.  Every output buffer is pre-filled (7.0 or NaN)
and its pad channels must keep the fill; pad channels of the input rows hold NaN, so reading one shows.  Every B = 2 case uses two
different samples and asserts that sample 1 equals, bit for bit, a B = 1 launch on sample 1's data alone.  Every case prints the
figures it is judged by."""
import pytest
import torch
import torch.nn.functional as F

import esclte_ref as L
import escreal_ref as R
import escrealm_ref as M
from helpers import check, dev_randn, fill_rows, need_trips, q, rnd

pytestmark = pytest.mark.gpu

DT = ["f32", "bf16"]
NAN = float("nan")

# ---- values / outputs the whole grid covers in ONE trip, as the launchers compute them --------------------------------------------
# hat_escrealm.hip hat_unshuffle_pad: `dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256)`, one row value per thread
UNSHUF_TRIP_VALUES = 8192 * 256
# hat_escrealm.hip hat_shuffle_planes: `dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256)`, one output value per thread
SHUFP_TRIP_OUTPUTS = 8192 * 256
# hat_escfp.hip hat_escfp_shuffle_bicubic: `dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256)`, one output value per thread
BICUBIC_TRIP_OUTPUTS = 8192 * 256
# hat_escreal.hip hat_dysample: `dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256)`, one output PIXEL (3 values) per thread
DYS_TRIP_PIXELS = 16384 * 256

# ---- the multi-trip frames: the smallest (up to the choice of factors) with three trips and a ragged last one --------------------
# f / s -> (B, rows, columns) of the row map.  B = 1: rows * columns * 3 f^2 just above two trips; B = 2: each sample just above ONE
# trip, so sample 1 starts inside the second.  The unshuffle's image is (f rows - pad) x (f columns - pad), both pads live.
UNSHUF_MT = {2: [(1, 547, 639, (1, 1)), (2, 373, 469, (1, 1))], 4: [(1, 281, 311, (3, 1))]}      # (B, Hb, Wb, (pad_h, pad_w))
SHUFP_MT = {2: [(1, 547, 639), (2, 373, 469)], 4: [(1, 281, 311)]}                                # (B, H, W)
BICUBIC_MT = {2: (2, 373, 469), 3: (2, 277, 281), 4: (2, 197, 223)}                               # (B, H, W): the entry takes a batch
DYS_MT = (2, 509, 517, 4)                                                                         # (B, H, W, s)


def unshuf_units(f, B, Hb, Wb):
    return B * Hb * Wb * 3 * f * f


def shuffle_units(s, B, H, W):
    return B * 3 * H * s * W * s


def dys_units(B, H, W, s):
    return B * H * s * W * s


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
    print(f"ESCREAL-EDGES {what} [{dtype}]: max-abs {err:.3e} rel {rel:.3e} (scale {float(r.abs().max()):.3g})")
    check(got, ref, dtype, what, f32_tol=f32_tol)


def _maps(rows, c, B, h, w):
    """(B, h*w, ld) rows -> (B, c, h, w) fp64 on the rows' device."""
    return rows[:, :, :c].double().transpose(1, 2).reshape(B, c, h, w)


def _nan_rows(x_bchw, ld, dev):
    """(B,C,H,W) -> fp32 device rows (B, H*W, ld) with NaN pad channels."""
    assert ld > x_bchw.shape[1]
    return fill_rows(x_bchw.permute(0, 2, 3, 1), ld, torch.float32, dev, NAN)


def _pads_keep(rows, c, fill, what):
    pad = rows[:, :, c:].float()
    assert rows.shape[2] > c and bool((torch.isnan(pad) if fill != fill else pad == fill).all()), what + ": pad channels written"


# ------------------------------------------------------------------------------------------------
# hat_unshuffle_pad, hat_shuffle_planes: three trips, two samples
# ------------------------------------------------------------------------------------------------
def _unshuffle(x, f, dev):
    """x (B,3,h,w) on the device -> the kernel's rows (B, Hb*Wb, 3 f^2 + 4), pre-filled with NaN."""
    B, _, h, w = x.shape
    Hb, Wb, cin = -(-h // f), -(-w // f), 3 * f * f
    rows = torch.full((B, Hb * Wb, cin + 4), NAN, device=dev)
    _ops().unshuffle_pad(x, rows, B=B, h=h, w=w, f=f, ld=cin + 4)
    torch.cuda.synchronize()
    return rows, Hb, Wb, cin


def _unshuffle_case(x, f, dev, what):
    B, _, h, w = x.shape
    rows, Hb, Wb, cin = _unshuffle(x, f, dev)
    want = F.pixel_unshuffle(F.pad(x, (0, Wb * f - w, 0, Hb * f - h), "reflect"), f)
    got = rows[:, :, :cin].transpose(1, 2).reshape(B, cin, Hb, Wb)
    bad = int((got != want).sum())
    print(f"ESCREAL-EDGES hat_unshuffle_pad {what}: {bad} of {want.numel()} values differ")
    assert torch.equal(got, want), what
    _pads_keep(rows, cin, NAN, "hat_unshuffle_pad rows")
    if B == 2:
        assert not torch.equal(rows[0, :, :cin], rows[1, :, :cin])
        rows1 = _unshuffle(x[1:2].contiguous(), f, dev)[0]
        assert torch.equal(rows[1:2, :, :cin], rows1[:, :, :cin]), "sample 1 of the B = 2 launch differs from a B = 1 launch on its image"


@pytest.mark.parametrize("case", [(f,) + c for f, cs in UNSHUF_MT.items() for c in cs], ids=lambda c: f"f{c[0]}_B{c[1]}_{c[2]}x{c[3]}")
def test_unshuffle_pad_multitrip(case):
    dev = _dev()
    f, B, Hb, Wb, (ph, pw) = case
    hi, lo = need_trips(unshuf_units(f, B, Hb, Wb), UNSHUF_TRIP_VALUES, 3, "hat_unshuffle_pad")
    h, w = Hb * f - ph, Wb * f - pw
    x = dev_randn(f"umt{case}", (B, 3, h, w), dev)
    _unshuffle_case(x, f, dev, f"/{f} {B}x{h}x{w} ({hi} / {lo} trips)")     # UNSHUF_TRIP_VALUES per trip


@pytest.mark.parametrize("f", [2, 4])
def test_unshuffle_pad_two_samples(f):
    """7 x 9: pads of 1 and 1 at f = 2, of 1 and 3 at f = 4."""
    dev = _dev()
    _unshuffle_case(rnd(f"u2s{f}", (2, 3, 7, 9)).to(dev), f, dev, f"/{f} 2x7x9")


def _shuffle(rows, B, H, W, s, ld, dev):
    y = torch.full((B, 3, H * s, W * s), NAN, device=dev)
    _ops().shuffle_planes(rows, y, B=B, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    return y


def _shuffle_case(rows, B, H, W, s, dev, what):
    """rows (B, H*W, 3 s^2 + 4) on the device, NaN pad channels."""
    n = 3 * s * s
    y = _shuffle(rows, B, H, W, s, n + 4, dev)
    want = F.pixel_shuffle(rows[:, :, :n].reshape(B, H, W, n).permute(0, 3, 1, 2), s)
    print(f"ESCREAL-EDGES hat_shuffle_planes {what}: {int((y != want).sum())} of {want.numel()} values differ")
    assert torch.equal(y, want), what
    if B == 2:
        assert not torch.equal(y[0], y[1])
        assert torch.equal(y[1:2], _shuffle(rows[1:2], 1, H, W, s, n + 4, dev)), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


@pytest.mark.parametrize("case", [(s,) + c for s, cs in SHUFP_MT.items() for c in cs], ids=lambda c: f"s{c[0]}_B{c[1]}_{c[2]}x{c[3]}")
def test_shuffle_planes_multitrip(case):
    dev = _dev()
    s, B, H, W = case
    hi, lo = need_trips(shuffle_units(s, B, H, W), SHUFP_TRIP_OUTPUTS, 3, "hat_shuffle_planes")
    n = 3 * s * s
    rows = torch.full((B, H * W, n + 4), NAN, device=dev)
    rows[:, :, :n] = dev_randn(f"smt{case}", (B, H * W, n), dev)
    _shuffle_case(rows, B, H, W, s, dev, f"x{s} {B}x{H}x{W} ({hi} / {lo} trips)")     # SHUFP_TRIP_OUTPUTS per trip


@pytest.mark.parametrize("s", [2, 3, 4])
def test_shuffle_planes_two_samples(s):
    dev = _dev()
    B, H, W = 2, 5, 7
    rows = _nan_rows(rnd(f"s2s{s}", (B, 3 * s * s, H, W)), 3 * s * s + 4, dev)
    _shuffle_case(rows, B, H, W, s, dev, f"x{s} 2x5x7")


# ------------------------------------------------------------------------------------------------
# hat_escfp_shuffle_bicubic: three trips, two samples
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sorted(BICUBIC_MT))
def test_escfp_shuffle_bicubic_multitrip(s):
    """test_shuffle_bicubic_matches_torch's reference (pixel_shuffle + F.interpolate bicubic) and bar (max-abs 1e-4), the reference
    in fp64 on the device."""
    dev, ops = _dev(), _ops()
    B, H, W = BICUBIC_MT[s]
    hi, lo = need_trips(shuffle_units(s, B, H, W), BICUBIC_TRIP_OUTPUTS, 3, "hat_escfp_shuffle_bicubic")
    n = 3 * s * s
    ld = n + 4
    rows = torch.full((B, H * W, ld), NAN, device=dev)
    rows[:, :, :n] = dev_randn(f"bmt{s}", (B, H * W, n), dev)
    g = torch.Generator(device=dev)
    g.manual_seed(500 + s)
    img = torch.rand((B, 3, H, W), generator=g, device=dev)
    ptab = ops.bicubic_phase_table(s).to(dev)

    def launch(rv, iv, b):
        y = torch.full((b, 3, H * s, W * s), NAN, device=dev)
        ops.escfp_shuffle_bicubic(rv, iv, ptab, y, B=b, H=H, W=W, s=s, ld=ld)     # BICUBIC_TRIP_OUTPUTS per trip
        torch.cuda.synchronize()
        return y

    y = launch(rows, img, B)
    want = F.pixel_shuffle(rows[:, :, :n].double().reshape(B, H, W, n).permute(0, 3, 1, 2), s) + F.interpolate(img.double(), scale_factor=s, mode="bicubic")
    assert bool(torch.isfinite(y).all()), "non-finite output"
    err = float((y.double() - want).abs().max())
    print(f"ESCREAL-EDGES hat_escfp_shuffle_bicubic x{s} {B}x{H}x{W} ({hi} / {lo} trips): max-abs {err:.3e} (scale {float(want.abs().max()):.3g})")
    assert err <= 1e-4, f"x{s}: max-abs {err:.3e}"
    assert not torch.equal(y[0], y[1])
    assert torch.equal(y[1:2], launch(rows[1:2], img[1:2], 1)), "sample 1 of the B = 2 launch differs from a B = 1 launch on its data"


# ------------------------------------------------------------------------------------------------
# hat_dysample: three trips at x4, two samples at x3
# ------------------------------------------------------------------------------------------------
def _dys_params(s):
    """Case c / d / e's DySample (x4 / x3 / x2): the folded pointwise weights (fp64, host), init_pos and end_conv's bias."""
    from super_resolution_amd import packing
    sd = R.d64(R.load_case({2: "e", 3: "d", 4: "c"}[s])[1])
    wd, bd = packing.dysample_fold(sd["to_img.offset.weight"], sd["to_img.offset.bias"], sd["to_img.scope.weight"], sd["to_img.end_conv.weight"])
    return sd, wd, bd, sd["to_img.init_pos"].reshape(-1), sd["to_img.end_conv.bias"]


def _dys_launch(rows, ip, bias, B, H, W, s, ld, dev):
    y = torch.full((B, 3, s * H, s * W), NAN, device=dev)
    _ops().dysample(rows, ip, bias, y, B=B, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    return y


def test_dysample_multitrip_two_samples():
    """x4, B = 2, 509 x 517: 8.42 M output pixels, three trips, sample 1 starts inside the second.  The rows are the fold of a
    seeded 64-channel map with case c's weights (offset and scope at std 0.3, as test_gpu_escreal.py), made on the device in fp32;
    the reference reads those rows.  The kernel forms its positions in fp32 as the reference's tensor ops do; near column 517 one
    ulp of a position is 6e-5 of a pixel, which is where the error against the exact fp64 positions comes from (measured: max-abs
    1.8e-4 at scale 3.98, relative L2 1.8e-5; 1.9e-6 on 9 x 13)."""
    dev = _dev()
    B, H, W, s = DYS_MT
    hi, lo = need_trips(dys_units(B, H, W, s), DYS_TRIP_PIXELS, 3, "hat_dysample")
    _, wd, bd, ip, bias = _dys_params(s)
    n = wd.shape[0]
    ld = n + 4
    rows = torch.full((B, H * W, ld), NAN, device=dev)
    rows[:, :, :n] = dev_randn("dysmt", (B, H * W, 64), dev) @ wd.float().t().to(dev) + bd.float().to(dev)
    ip, bias = ip.float().to(dev), bias.float().to(dev)
    y = _dys_launch(rows, ip, bias, B, H, W, s, ld, dev)     # DYS_TRIP_PIXELS per trip
    want = R.dysample_from_rows(rows, ip, bias, H, W, s, band=32)
    moved = (rows[:, :, :8 * s * s].double() * torch.sigmoid(rows[:, :, 8 * s * s:16 * s * s].double()) * 0.5).abs()
    print(f"ESCREAL-EDGES hat_dysample x{s} {B}x{H}x{W} ({hi} / {lo} trips): offsets move samples by up to {float(moved.max()):.2f} px, "
          f"{float((moved > 1).double().mean()):.3f} of them by more than one")
    assert float(moved.max()) > 2.0, "no sample leaves its own pixel's neighbourhood"
    _judge(y, want, "f32", f"hat_dysample x{s} {B}x{H}x{W}")
    assert not torch.equal(y[0], y[1])
    assert torch.equal(y[1:2], _dys_launch(rows[1:2], ip, bias, 1, H, W, s, ld, dev)), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


def test_dysample_two_samples_x3():
    dev = _dev()
    B, H, W, s = 2, 9, 13, 3
    sd, wd, bd, ip, bias = _dys_params(s)
    feat = rnd("dys2s", (B, 64, H, W)).double()
    rows_h = F.conv2d(feat, wd[:, :, None, None], bd).float()
    ld = wd.shape[0] + 4
    rows = _nan_rows(rows_h, ld, dev)
    ip, bias = ip.float().to(dev), bias.float().to(dev)
    y = _dys_launch(rows, ip, bias, B, H, W, s, ld, dev)
    _judge(y, R.dysample_from_rows(rows, ip, bias, H, W, s), "f32", f"hat_dysample x{s} {B}x{H}x{W}")
    want = torch.cat([R.head_dysample(feat[b:b + 1], sd, s) for b in range(B)])      # the head itself, from the map
    _judge(y, want, "f32", f"hat_dysample x{s} {B}x{H}x{W} vs head_dysample")
    assert not torch.equal(y[0], y[1])
    assert torch.equal(y[1:2], _dys_launch(rows[1:2], ip, bias, 1, H, W, s, ld, dev)), "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


# ------------------------------------------------------------------------------------------------
# hat_escreal_skip: batch, one tile, frames narrower than the window
# ------------------------------------------------------------------------------------------------
def _skip_sd():
    return {"skip.0.weight": rnd("s0w", (128, 3, 1, 1)), "skip.0.bias": rnd("s0b", (128,)),
            "skip.1.weight": rnd("s1w", (128, 1, 7, 7), std=1 / 7), "skip.1.bias": rnd("s1b", (128,)),
            "skip.3.weight": rnd("s3w", (64, 128, 1, 1), std=128 ** -0.5), "skip.3.bias": rnd("s3b", (64,))}


def _skip_launch(ps, x, rr, dtype, dev):
    """x (B,3,H,W) on the device, rr rows (B, H*W, 68) or None -> out rows (B, H*W, 72) pre-filled with 7.0."""
    ops = _ops()
    B, _, H, W = x.shape
    out = torch.full((B, H * W, 72), 7.0, device=dev)
    ops.escreal_skip(ps, x, out, B=B, H=H, W=W, dtype=ops.DTYPE_CODE[dtype], r=rr, ldr=68, ldo=72)
    torch.cuda.synchronize()
    return out


def _skip_case(dtype, B, H, W, with_r, dev):
    ops = _ops()
    sd = _skip_sd()
    x, r = q(rnd(f"ex{B}x{H}x{W}", (B, 3, H, W)), dtype), rnd(f"er{B}x{H}x{W}", (B, 64, H, W))
    ps = ops.pack_escreal_skip(sd, "skip", ops.DTYPE_CODE[dtype], dev)
    xd, rr = x.to(dev), _nan_rows(r, 68, dev) if with_r else None
    out = _skip_launch(ps, xd, rr, dtype, dev)
    want = R.skip_branch(x.double(), R.d64(sd)) + (r.double() if with_r else 0.0)
    _judge(_maps(out, 64, B, H, W), want, dtype, f"hat_escreal_skip {B}x{H}x{W}{' r' if with_r else ''}")
    _pads_keep(out, 64, 7.0, "hat_escreal_skip out")
    if B == 2:
        assert not torch.equal(out[0], out[1])
        out1 = _skip_launch(ps, xd[1:2].contiguous(), rr[1:2] if with_r else None, dtype, dev)
        assert torch.equal(out[1:2], out1), "sample 1 of the B = 2 launch differs from a B = 1 launch on its data"


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "r"])
@pytest.mark.parametrize("dtype", DT)
def test_escreal_skip_two_samples(dtype, with_r):
    _skip_case(dtype, 2, 5, 7, with_r, _dev())


#                                  8x8: exactly one 64-pixel tile;  4x37 / 37x4: narrower than the 7-tap window on one axis (every pixel reflects on both
#                                  sides of it at once), 148 pixels: two full tiles and a ragged third
@pytest.mark.parametrize("hw", [(8, 8), (4, 37), (37, 4)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("dtype", DT)
def test_escreal_skip_tile_geometry(dtype, hw):
    _skip_case(dtype, 1, hw[0], hw[1], True, _dev())


# ------------------------------------------------------------------------------------------------
# hat_escrealm_skip: batch, the one-pixel overhang, the minimum height, exact tile multiples
# ------------------------------------------------------------------------------------------------
def _wide_sd(cin):
    return {"skip.1.weight": rnd(f"m1w{cin}", (128, cin, 1, 1), std=cin ** -0.5), "skip.1.bias": rnd("m1b", (128,)),
            "skip.2.weight": rnd("m2w", (128, 1, 7, 7), std=1 / 7), "skip.2.bias": rnd("m2b", (128,)),
            "skip.4.weight": rnd("m4w", (64, 128, 1, 1), std=128 ** -0.5), "skip.4.bias": rnd("m4b", (64,))}


def _wide_launch(ps, xr, rr, dtype, B, H, W, cin, dev):
    ops = _ops()
    out = torch.full((B, H * W, 72), 7.0, device=dev)
    ops.escrealm_skip(ps, xr, out, B=B, H=H, W=W, dtype=ops.DTYPE_CODE[dtype], ldx=cin + 4, r=rr, ldr=68, ldo=72)
    torch.cuda.synchronize()
    return out


def _wide_case(dtype, cin, B, H, W, dev):
    """With r; x rows at ldx = cin + 4 with NaN pad channels: the f32x4 halo load one step past cin would show."""
    ops = _ops()
    sd = _wide_sd(cin)
    x, r = rnd(f"wx{cin}_{B}x{H}x{W}", (B, cin, H, W)), rnd(f"wr{B}x{H}x{W}", (B, 64, H, W))
    ps = ops.pack_escrealm_skip(sd, "skip", ops.DTYPE_CODE[dtype], dev)
    xr, rr = _nan_rows(x, cin + 4, dev), _nan_rows(r, 68, dev)
    out = _wide_launch(ps, xr, rr, dtype, B, H, W, cin, dev)
    want = M.skip_branch(x.double(), M.d64(sd), first=1) + r.double()
    _judge(_maps(out, 64, B, H, W), want, dtype, f"hat_escrealm_skip {cin} {B}x{H}x{W} r")
    _pads_keep(out, 64, 7.0, "hat_escrealm_skip out")
    if B == 2:
        assert not torch.equal(out[0], out[1])
        assert torch.equal(out[1:2], _wide_launch(ps, xr[1:2], rr[1:2], dtype, 1, H, W, cin, dev)), \
            "sample 1 of the B = 2 launch differs from a B = 1 launch on its rows"


@pytest.mark.parametrize("cin", [12, 48])
@pytest.mark.parametrize("dtype", DT)
def test_escrealm_skip_two_samples(dtype, cin):
    _wide_case(dtype, cin, 2, 10, 16, _dev())


#                                  9x9: a one-pixel overhang on both axes, the reflected halo coordinate of the dropped pixels goes negative and is clamped;
#                                  4x17: the minimum height, three tile columns, the last one pixel wide;  16x8: exact multiples of the tile
@pytest.mark.parametrize("hw", [(9, 9), (4, 17), (16, 8)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("cin", [12, 48])
@pytest.mark.parametrize("dtype", DT)
def test_escrealm_skip_tile_geometry(dtype, cin, hw):
    _wide_case(dtype, cin, 1, hw[0], hw[1], _dev())


# ------------------------------------------------------------------------------------------------
# hat_lte_query: the affine in explicit mode, coef and freq apart, one-pixel and one-column maps, a grid below the map
# ------------------------------------------------------------------------------------------------
LTE_SMALL_MAPS = {(1, 1): (5, 6), (3, 1): (8, 3)}   # map -> the grid queried on it ((5, 6) on 1 x 1: x5, the cell is clipped at scale_max)
LTE_EXPLICIT_Q = 33


def _lte():
    import test_gpu_esclte as T
    return T


def _lte_grid(ops, pl, coef, freq, inp, hw, cell, kw):
    h, w = hw
    planes = torch.full((3, h, w), NAN, device=inp.device)
    ops.lte_query(pl, coef, freq, inp, planes, grid=(h, w), cell_yx=(float(cell[0, 0]), float(cell[0, 1])), out_affine=(0.5, 0.5), **kw)
    torch.cuda.synchronize()
    return (planes.permute(1, 2, 0).reshape(-1, 3) - 0.5) / 0.5


def _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw, **more):
    out = torch.full((coord.shape[0], 3), NAN, device=inp.device)
    ops.lte_query(pl, coef, freq, inp, out, coord=coord.to(inp.device), cell=cell.to(inp.device), **dict(kw, **more))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DT)
def test_lte_explicit_mode_applies_the_affine(dtype):
    T = _lte()
    H, W = 5, 7
    ops, pl, coef, freq, inp, kw = T.device_head(dtype, H, W)
    coord, cell, _ = T.head_ref(H, W, ("scatter", L.N_SCATTER))
    plain = _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw)
    aff = _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw, out_affine=(0.5, 0.5))
    _judge(aff, plain.double() * 0.5 + 0.5, "f32", f"lte_query explicit, affine (0.5, 0.5) [{dtype} kernel]")
    assert not torch.equal(aff, plain)


@pytest.mark.parametrize("dtype", DT)
def test_lte_coef_and_freq_in_buffers_of_their_own(dtype):
    """ldc 260, ldf 264, NaN pad channels, both addressing modes, against the interleaved 512-wide layout (fp32: bit-equal, no
    operation's order depends on a leading dimension) and against the fp64 head."""
    T = _lte()
    H, W = 5, 7
    ops, pl, rows, freq_il, inp, kw = T.device_head(dtype, H, W)
    c, f, _ = T.head_case(H, W)
    coef = fill_rows(c.permute(0, 2, 3, 1), 260, torch.float32, inp.device, NAN)[0]
    freq = fill_rows(f.permute(0, 2, 3, 1), 264, torch.float32, inp.device, NAN)[0]
    kw2 = dict(kw, ldc=260, ldf=264)
    coord, cell, y = T.head_ref(H, W, ("scatter", L.N_SCATTER))
    gc, gcell, gy = T.head_ref(H, W, ("grid", (11, 13)))
    for what, got, il, ref in (("explicit", _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw2), _lte_explicit(ops, pl, rows, freq_il, inp, coord, cell, kw), y),
                               ("grid 11x13", _lte_grid(ops, pl, coef, freq, inp, (11, 13), gcell, kw2), _lte_grid(ops, pl, rows, freq_il, inp, (11, 13), gcell, kw), gy)):
        print(f"ESCREAL-EDGES lte_query {what}, coef / freq apart [{dtype}]: max-abs vs interleaved {float((got - il).abs().max()):.3e}")
        if dtype == "f32":
            assert torch.equal(got, il), f"{what}: the split layout differs from the interleaved one"
        else:
            check(got, il, "bf16", f"lte_query {what}, split vs interleaved")
        T.kernel_bar(got, ref, dtype, f"lte_query {what}, ldc 260 / ldf 264 on {H}x{W}")
        if dtype == "bf16":
            T.mlp_bar(got, H, W, ("scatter", L.N_SCATTER) if what == "explicit" else ("grid", (11, 13)), f"lte_query {what}, ldc 260 / ldf 264")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", list(LTE_SMALL_MAPS), ids=lambda m: f"{m[0]}x{m[1]}")
def test_lte_one_pixel_and_one_column_maps(hw, dtype):
    """1 x 1: all four shifts clamp to the one pixel and the four areas are equal;  3 x 1: one column.  Explicit (33 scattered
    coordinates with -1 and 1 on both axes) and grid."""
    T = _lte()
    H, W = hw
    ops, pl, coef, freq, inp, kw = T.device_head(dtype, H, W)
    key = ("scatter", LTE_EXPLICIT_Q)
    coord, cell, y = T.head_ref(H, W, key)
    got = _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw)
    T.kernel_bar(got, y, dtype, f"lte_query explicit Q={LTE_EXPLICIT_Q} on {H}x{W}")
    if dtype == "bf16":
        T.mlp_bar(got, H, W, key, f"lte_query explicit Q={LTE_EXPLICIT_Q} on {H}x{W}")
    g = LTE_SMALL_MAPS[hw]
    _, gcell, gy = T.head_ref(H, W, ("grid", g))
    got = _lte_grid(ops, pl, coef, freq, inp, g, gcell, kw)
    T.kernel_bar(got, gy, dtype, f"lte_query grid {g[0]}x{g[1]} on {H}x{W}")
    if dtype == "bf16":
        T.mlp_bar(got, H, W, ("grid", g), f"lte_query grid {g[0]}x{g[1]} on {H}x{W}")


@pytest.mark.parametrize("dtype", DT)
def test_lte_grid_smaller_than_the_map(dtype):
    """3 x 4 on the 5 x 7 map: a cell larger than a feature pixel."""
    T = _lte()
    H, W, g = 5, 7, (3, 4)
    ops, pl, coef, freq, inp, kw = T.device_head(dtype, H, W)
    coord, cell, y = T.head_ref(H, W, ("grid", g))
    assert float(cell[0, 0]) * H > 2.0 and float(cell[0, 1]) * W > 2.0      # in feature pixels (a pixel is 2 / n wide)
    got = _lte_grid(ops, pl, coef, freq, inp, g, cell, kw)
    T.kernel_bar(got, y, dtype, f"lte_query grid 3x4 on {H}x{W}")
    check(got, _lte_explicit(ops, pl, coef, freq, inp, coord, cell, kw), "f32", f"grid mode vs explicit mode 3x4 on {H}x{W} [{dtype}]")
    if dtype == "bf16":
        T.mlp_bar(got, H, W, ("grid", g), f"lte_query grid 3x4 on {H}x{W}")
