"""10 / 12 / 16-bit 4:2:0 on the GPU: P010 / P012 / P016 / yuv420p1xle frames in and out through the kernels, the engine, the
modules, the plans, the C example, the frame-sequence generator and the video tool.  As in tests/test_gpu_yuv.py every
comparison is an equality against super_resolution_amd/yuv.py, the numpy definition (tests/test_yuv_deep_cpu.py ties its deep
part to the 8-bit one): no tolerance and no pixels left out.  uint16 tensors are compared through their int16 view."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import META, W_SEED
from super_resolution_amd import synth, y4m, yuv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HATS = dict(in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01, overlap_ratio=0.5,
            img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
MATRICES = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True), ("bt2020nc", False)]
WIDTHS = [(10, True), (10, False), (12, False), (16, False)]      # (depth, msb)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _net(arch, name, dtype, dev, **kw):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    cfg = META["cfgs"][name] if isinstance(name, str) else name
    net = build_network(dict(type=arch, compute_dtype=dtype, **dict(cfg, **kw))).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    return net.to(dev)


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _up(a, dev):
    """numpy uint8 / uint16 -> device tensor of the same dtype"""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def _down(t):
    t = t.contiguous() if t.dtype != torch.uint16 else _raw(t).contiguous()
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _words(seed, shape, depth, msb):
    """stored samples: every word value may occur for an MSB container (low bits set) and for 16 bits; LSB containers get words
    above the range too (one in eight)"""
    rng = np.random.default_rng(seed)
    if depth == 16 or msb:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    w = rng.integers(0, 1 << depth, shape, dtype=np.uint16)
    over = rng.integers(0, 8, shape) == 0
    return np.where(over, rng.integers(1 << depth, 65536, shape, dtype=np.uint16), w)


def _frames(seed, shape, depth=8, fmt="i420"):
    """random codes of `depth` bits as the stored samples of layout `fmt` (MSB-aligned words for nv12 / nv21)"""
    if depth == 8:
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    return yuv.encode(np.random.default_rng(seed).integers(0, 1 << depth, shape, dtype=np.uint16), depth, fmt)


def _pitched16(B, h, w, fmt, dev, fill, y_extra=5, c_extra=3):
    """uint16 device buffers for a (B, h, w) frame: Y rows w + y_extra words apart and chroma rows c_extra words longer than a
    chroma row, each made odd in words, so the byte pitches are even and no multiple of 4.  Returns buffers and views."""
    odd = lambda n: n + 1 - n % 2
    ybuf = torch.full((B, h, odd(w + y_extra)), fill, dtype=torch.int16, device=dev).view(torch.uint16)
    if fmt == "i420":
        cbuf = torch.full((2, B, h // 2, odd(w // 2 + c_extra)), fill, dtype=torch.int16, device=dev).view(torch.uint16)
        cb, cr = cbuf[0, :, :, :w // 2], cbuf[1, :, :, :w // 2]
    else:
        cbuf = torch.full((B, h // 2, odd(w + c_extra)), fill, dtype=torch.int16, device=dev).view(torch.uint16)
        a, b = cbuf[:, :, 0:w:2], cbuf[:, :, 1:w:2]
        cb, cr = (a, b) if fmt == "nv12" else (b, a)
    return ybuf, cbuf, (ybuf[:, :, :w], cb, cr)


def _guards_intact(ybuf, cbuf, w, fmt, fill):
    if not bool((_raw(ybuf)[:, :, w:] == fill).all()):
        return False
    return bool((_raw(cbuf)[..., (w // 2 if fmt == "i420" else w):] == fill).all())


def _put(view, a):
    _raw(view).copy_(torch.from_numpy(a.view(np.int16)).to(view.device))


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("pad", [(0, 0), (6, 0), (0, 6), (6, 6)])
def test_yuv420p16_to_planes_is_the_definition(pad, fmt):
    dev = _dev()
    from super_resolution_amd import ops
    B, h, w = 2, 38, 302                                        # not multiples of the 256-pixel workgroup row
    Hp, Wp = h + pad[0], w + pad[1]
    big = torch.full((B * 3 * Hp * Wp + 64,), -7.0, device=dev)
    dst = big[32:-32].view(B, 3, Hp, Wp)
    for depth, msb in WIDTHS:
        shift = 16 - depth if msb else 0
        Y, Cb, Cr = (_words(s, sh, depth, msb) for s, sh in ((1, (B, h, w)), (2, (B, h // 2, w // 2)), (3, (B, h // 2, w // 2))))
        if depth == 10:
            for a in (Y, Cb, Cr):
                a.reshape(-1)[-1024:] = np.arange(1024, dtype=np.uint16) << shift       # every 10-bit code is present
        if not msb and depth < 16:
            assert (Y > (1 << depth) - 1).any() and (Cb > (1 << depth) - 1).any(), "out-of-range LSB words are present"
        k = depth - 8
        Y[0, 0, 0:2], Cb[0, 0, 0], Cr[0, 0, 0] = (16 << k) << shift, (128 << k) << shift, (16 << k) << shift     # R below 0
        Y[0, 0, 2:4], Cb[0, 0, 1], Cr[0, 0, 1] = (235 << k) << shift, (128 << k) << shift, (240 << k) << shift   # R above 1
        frame = yuv.join(Y, Cb, Cr, fmt, depth, msb)
        ybuf, cbuf, (y, cb, cr) = _pitched16(B, h, w, fmt, dev, 0)
        _put(y, Y), _put(cb, Cb), _put(cr, Cr)
        assert (2 * y.stride(1)) % 4 == 2 and (2 * cb.stride(1)) % 4 == 2 and cb.stride(2) == (1 if fmt == "i420" else 2)
        for matrix, full in MATRICES:
            to_rgb, _ = yuv.csc(matrix, full, depth)
            big.fill_(-7.0)
            ops.yuv420_to_planes(y, cb, cr, dst, to_rgb, depth=depth, msb=msb)
            torch.cuda.synchronize()
            ref = yuv.yuv420_to_planes(frame, fmt=fmt, matrix=matrix, full_range=full, pad=pad, depth=depth, msb=msb)
            if not full:
                assert ref[0, 0, 0, 0] == 0.0 and ref[0, 0, 0, 2] == 1.0, "the two triples are clamped"
            assert np.array_equal(dst.cpu().numpy(), ref), (depth, msb, matrix, full)
            assert bool((big[:32] == -7.0).all()) and bool((big[-32:] == -7.0).all()), "floats outside the planes are not the kernel's"


# ---------------------------------------------------------------------------------------------- 2
def _special_planes(B, Hs, Ws):
    """As test_gpu_yuv._special_planes builds them for bytes: zeros of both signs, 1 and its successor, the infinities, every
    k / 255, and — for the 10-bit limited luma, whose code is (16 + 219 v) * 4 — values that land on and beside rounding ties:
    v = (c + 0.5 - 64) / 876 with its fp32 neighbours; uniform values in [-0.5, 1.5) elsewhere.  NaN-free."""
    g = torch.Generator().manual_seed(5)
    t = torch.rand(B * 3 * Hs * Ws, generator=g) * 2.0 - 0.5
    k = torch.arange(256, dtype=torch.float32)
    c = torch.arange(64, 940, 3, dtype=torch.float32)
    half = (c + 0.5 - 64.0) / 876.0
    up, down = torch.nextafter(half, torch.tensor(2.0)), torch.nextafter(half, torch.tensor(-1.0))
    one = torch.tensor(1.0)
    sp = torch.cat([torch.tensor([-0.0, 0.0, 1.0, float(torch.nextafter(one, torch.tensor(2.0))), float("inf"), float("-inf")]),
                    k / 255.0, half, up, down])
    assert sp.numel() <= Hs * Ws - 200
    t = t.reshape(B, 3, Hs * Ws)
    for ch in range(3):
        t[0, ch, 100 * ch:100 * ch + sp.numel()] = sp
    # grey runs: r = g = b = a tie value, so that Y itself (not one term of it) sits on the tie
    n = half.numel()
    t[1, :, :n] = half
    t[1, :, n:2 * n] = up
    assert not bool(torch.isnan(t).any())
    return t.reshape(B, 3, Hs, Ws)


@pytest.fixture(scope="module")
def special():
    return _special_planes(2, 31, 61)


@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("crop", [(30, 60), (26, 56), (30, 50)])
def test_planes_to_yuv420p16_is_the_definition(crop, fmt, special):
    dev = _dev()
    from super_resolution_amd import ops
    B, (ho, wo) = 2, crop
    src = special.to(dev)
    for depth, msb in WIDTHS:
        for matrix, full in MATRICES[1:4] if depth != 10 else MATRICES:
            _, from_rgb = yuv.csc(matrix, full, depth)
            ref = yuv.planes_to_yuv420(special.numpy(), fmt=fmt, matrix=matrix, full_range=full, crop=crop, out_depth=depth, msb=msb)
            # odd word pitches: Y rows start 2 (mod 4) bytes apart, so aligned and misaligned 8-byte segments alternate
            ybuf, cbuf, (y, cb, cr) = _pitched16(B, ho, wo, fmt, dev, 99)
            ops.planes_to_yuv420(src, y, cb, cr, from_rgb, depth=depth, msb=msb)
            packed = torch.full((B,) + yuv.frame_shape(ho, wo), 99, dtype=torch.int16, device=dev).view(torch.uint16)   # packed rows: 8-byte Y stores
            assert packed.data_ptr() % 8 == 0 and y.data_ptr() % 8 == 0 and (2 * y.stride(1)) % 8 != 0
            ops.planes_to_yuv420(src, *ops.yuv420_views(packed, fmt), from_rgb, depth=depth, msb=msb)
            torch.cuda.synchronize()
            got = yuv.join(_down(y), _down(cb), _down(cr), fmt, depth, msb)
            assert np.array_equal(got, ref), (depth, msb, matrix, full)
            assert np.array_equal(_down(packed), ref), (depth, msb, matrix, full)
            assert _guards_intact(ybuf, cbuf, wo, fmt, 99), "words between the rows are not the kernel's"


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("shape", [(24, 16), (24, 48), (72, 5120)], ids=["24x16", "24x48", "72x5120"])
def test_conv3x3_to_yuv420p16_equals_planes_then_convert(shape):
    """The shapes of the 8-bit test: 24 rows are three 8-row bands, so the carried row pair crosses the three-row unroll; 48
    columns are several strips; at 72 x 5120 the planes geometry has 9 rows per band and the round-up to even is exercised."""
    dev = _dev()
    from super_resolution_amd import ops
    from super_resolution_amd.engine import RGB_MEAN
    H, W = shape
    B = 2
    g = torch.Generator().manual_seed(W)
    x = (torch.randn(B, H, W, 64, generator=g)).to(torch.bfloat16).to(dev)
    wl = torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0)
    bl = torch.randn(3, generator=g) * 0.1
    wpk, b8 = ops.pack_cab_squeeze(wl, bl, dev)
    kw = dict(B=B, H=H, W=W, C_=64, ldx=64, out_scale=0.5, mean=RGB_MEAN, dtype=ops.HAT_BF16)
    planes = torch.empty(B, 3, H, W, device=dev)
    ops.conv3x3_to_planes(x, wpk, b8, planes, n_out=3, **kw)
    torch.cuda.synchronize()
    inside = float(((planes > 0) & (planes < 1)).float().mean())
    assert 0.3 < inside < 0.95, inside
    if W == 5120:
        assert -(-H // (3072 // ((W + 13) // 14))) == 9, "the planes geometry has an odd band height here"
    for ho, wo in ((H, W), (H - 4, W - 6), (H - 2, (W // 14) * 14 if W > 16 else 14), (2, 2)):
        for depth, msb, fmt, (matrix, full) in ((10, True, "nv12", ("bt601", False)), (12, False, "nv21", ("bt2020nc", False)), (16, False, "i420", ("bt709", True))):
            _, m = yuv.csc(matrix, full, depth)
            ref = torch.empty((B,) + yuv.frame_shape(ho, wo), dtype=torch.uint16, device=dev)
            ops.planes_to_yuv420(planes, *ops.yuv420_views(ref, fmt), m, depth=depth, msb=msb)
            ybuf, cbuf, (y, cb, cr) = _pitched16(B, ho, wo, fmt, dev, 77, y_extra=1, c_extra=1)
            ops.conv3x3_to_yuv420(x, wpk, b8, y, cb, cr, from_rgb=m, depth=depth, msb=msb, **kw)
            torch.cuda.synchronize()
            ry, rcb, rcr = ops.yuv420_views(ref, fmt)
            assert torch.equal(_raw(y), _raw(ry)), (ho, wo, depth, fmt, "Y")
            assert torch.equal(_raw(cb), _raw(rcb)) and torch.equal(_raw(cr), _raw(rcr)), (ho, wo, depth, fmt, "chroma")
            assert _guards_intact(ybuf, cbuf, wo, fmt, 77)
    # the u8 and 8-bit yuv epilogues give what they gave on the same inputs
    ref8 = torch.empty(B, H - 3, W - 5, 3, dtype=torch.uint8, device=dev)
    ops.planes_to_u8(planes, ref8)
    out8 = torch.empty_like(ref8)
    ops.conv3x3_to_u8(x, wpk, b8, out8, h_out=H - 3, w_out=W - 5, bgr=False, **kw)
    _, m8 = yuv.csc("bt601", False)
    refy = torch.empty((B,) + yuv.frame_shape(H - 4, W - 6), dtype=torch.uint8, device=dev)
    ops.planes_to_yuv420(planes, *ops.yuv420_views(refy, "nv12"), m8)
    outy = torch.empty_like(refy)
    ops.conv3x3_to_yuv420(x, wpk, b8, *ops.yuv420_views(outy, "nv12"), from_rgb=m8, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out8, ref8) and torch.equal(outy, refy)
    assert np.array_equal(refy.cpu().numpy(), yuv.planes_to_yuv420(planes.cpu().numpy(), crop=(H - 4, W - 6)))


# ---------------------------------------------------------------------------------------------- 4
def _composition(net, frames, ws, s, dev, *, fmt, matrix, full_range, depth, out_depth, msb=None):
    """host yuv420_to_planes (with the reflect-pad) -> this build's forward -> crop -> host planes_to_yuv420"""
    h, w = yuv.frame_size(frames.shape)
    pad = ((ws - h % ws) % ws, (ws - w % ws) % ws)
    x = yuv.yuv420_to_planes(frames, fmt=fmt, matrix=matrix, full_range=full_range, pad=pad, depth=depth, msb=msb)
    y = net(torch.from_numpy(x).to(dev)).cpu().numpy()
    return yuv.planes_to_yuv420(y, fmt=fmt, matrix=matrix, full_range=full_range, crop=(s * h, s * w), out_depth=out_depth, msb=msb)


NETS = [("HAT", "tiny_x2", (1, 38, 54)), ("HAT", "tiny_x4", (2, 38, 54)), ("HAT", "tiny_x3", (1, 16, 10)), ("HATX", "hatx_tiny_plain_x2", (2, 38, 54))]
ROUTES = [(10, 10, "nv12", ("bt601", False)), (8, 10, "nv12", ("bt709", True)), (10, 8, "i420", ("bt2020nc", False)),
          (16, 16, "i420", ("bt709", False)), (12, 12, "nv21", ("bt601", True))]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", NETS, ids=[f"{c[1]}_B{c[2][0]}_{c[2][1]}x{c[2][2]}" for c in NETS])
def test_forward_yuv420_deep_is_the_composition(case, dtype):
    dev = _dev()
    arch, name, (B, h, w) = case
    cfg = META["cfgs"][name]
    ws, s = cfg["window_size"], cfg["upscale"]
    net = _net(arch, name, dtype, dev)
    eng = net.engine()
    fused = dtype == "bf16" and (s * -(-w // ws) * ws) % 16 == 0
    for depth, out_depth, fmt, (matrix, full) in ROUTES:
        frames = _frames(h * w + B + depth, (B,) + yuv.frame_shape(h, w), depth, fmt)
        kw = dict(fmt=fmt, matrix=matrix, full_range=full, depth=depth, out_depth=out_depth)
        ref = _composition(net, frames, ws, s, dev, **kw)
        d = _up(frames, dev)
        counts = (eng.yuv_fused_calls, eng.yuv_planes_calls)
        out = net.forward_yuv420(d, **kw)
        assert out.dtype == (torch.uint8 if out_depth == 8 else torch.uint16) and tuple(out.shape) == (B,) + yuv.frame_shape(s * h, s * w)
        assert np.array_equal(_down(out), ref), (depth, out_depth, fmt)
        assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (counts[0] + int(fused), counts[1] + int(not fused)), "the width rule is the 8-bit one"
        mine = torch.zeros(out.shape, dtype=torch.int16 if out_depth != 8 else torch.uint8, device=dev)
        mine = mine.view(torch.uint16) if out_depth != 8 else mine
        got = None                                               # (the previous route's result is released before the count)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        got = net.forward_yuv420(d, out=mine, **kw)
        torch.cuda.synchronize()
        assert got is mine and np.array_equal(_down(mine), ref), "out= is filled with the same words"
        assert torch.cuda.memory_allocated(dev) == before, "with out= the call keeps nothing"
        if fused:
            assert torch.cuda.max_memory_allocated(dev) == before, "with out= and the fused epilogue the call allocates nothing"
    if B == 1:                                                   # (3h/2, w) is accepted as one frame; out_depth defaults to depth
        f10 = _frames(3, yuv.frame_shape(h, w), 10)
        a = net.forward_yuv420(_up(f10, dev), fmt="i420", depth=10)
        assert a.dtype == torch.uint16 and np.array_equal(_down(a), _composition(net, f10[None], ws, s, dev, fmt="i420", matrix="bt601", full_range=False, depth=10, out_depth=10))


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ten_bit_frame_of_eight_bit_codes_gives_the_eight_bit_result(dtype):
    dev = _dev()
    net = _net("HAT", "tiny_x2", dtype, dev)
    f = _frames(11, (2,) + yuv.frame_shape(38, 54))
    for fmt in ("nv12", "i420"):
        want = net.forward_yuv420(torch.from_numpy(f).to(dev), fmt=fmt)
        deep = f.astype(np.uint16) * 4                           # the 10-bit limited-range code of every sample
        words = deep << 6 if fmt == "nv12" else deep             # nv12 is MSB-aligned by default
        got = net.forward_yuv420(_up(words, dev), fmt=fmt, depth=10, out_depth=8)
        assert got.dtype == torch.uint8 and torch.equal(got, want), fmt


# ---------------------------------------------------------------------------------------------- 6
def test_forward_yuv420_deep_refusals():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "f32", dev)
    z8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dev)
    z16 = lambda *shape: torch.zeros(*shape, dtype=torch.int16, device=dev).view(torch.uint16)
    with pytest.raises(TypeError, match="uint16"):
        net.forward_yuv420(z8(1, 24, 20), depth=10)              # dtype against depth
    with pytest.raises(TypeError, match="uint8"):
        net.forward_yuv420(z16(1, 24, 20))
    with pytest.raises(TypeError, match="uint8"):
        net.forward_yuv420(torch.zeros(1, 24, 20, device=dev), depth=10)
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv420(z16(1, 24, 20), depth=10, out=z8(1, 48, 40))
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv420(z8(1, 24, 20), out_depth=10, out=z8(1, 48, 40))
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv420(z16(1, 24, 20), depth=10, out=z16(1, 48, 42))
    with pytest.raises(RuntimeError, match="depth"):
        net.forward_yuv420(z16(1, 24, 20), depth=9)
    with pytest.raises(RuntimeError, match="depth"):
        net.forward_yuv420(z8(1, 24, 20), out_depth=14)
    with pytest.raises(RuntimeError, match="matrix"):
        net.forward_yuv420(z16(1, 24, 20), depth=10, matrix="bt2020")
    with pytest.raises(RuntimeError, match="even"):
        net.forward_yuv420(z16(1, 24, 21), depth=10)
    with pytest.raises(RuntimeError, match="even"):
        net.forward_yuv420(z16(1, 25, 20), depth=12)
    with pytest.raises(RuntimeError, match="GPU"):
        net.forward_yuv420(torch.zeros(1, 24, 20, dtype=torch.uint16), depth=10)
    net1 = _net("HAT", "tiny_x2", "f32", dev, in_chans=1)
    with pytest.raises(RuntimeError, match="in_chans"):
        net1.forward_yuv420(z16(1, 24, 16), depth=10)


# ---------------------------------------------------------------------------------------------- 7
PLANS = [("HAT", "hats_1g_x4", "bf16", (1, 3, 32, 48), (28, 42), "nv12", 10, 10), ("HATX", "hatx_tiny_plain_x2", "f32", (2, 3, 16, 24), (16, 24), "i420", 8, 10)]


@pytest.mark.parametrize("case", PLANS, ids=["hats_bf16_p010", "hatx_f32_B2_8to10"])
def test_plan_forward_yuv420_deep(case, tmp_path):
    dev = _dev()
    from super_resolution_amd import _lib, ops, plan
    arch, name, dtype, shape, small, fmt, depth, out_depth = case
    B, _, H, W = shape
    s = META["cfgs"][name]["upscale"]
    net = _net(arch, name, dtype, dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, shape, path)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    out_dt = torch.uint8 if out_depth == 8 else torch.uint16
    for h, w in {(H, W), small}:
        frames = _up(_frames(h + w, (B,) + yuv.frame_shape(h, w), depth, fmt), dev)
        for matrix, full in (("bt601", False), ("bt2020nc", True)):
            kw = dict(fmt=fmt, matrix=matrix, full_range=full, depth=depth, out_depth=out_depth)
            ref = net.forward_yuv420(frames, **kw)
            out = torch.full((B,) + yuv.frame_shape(s * h, s * w), 9, dtype=torch.int16, device=dev).view(out_dt) if out_depth != 8 else \
                torch.full((B,) + yuv.frame_shape(s * h, s * w), 9, dtype=torch.uint8, device=dev)
            p.forward_yuv420(frames, out, stream=stream, **kw)
            torch.cuda.synchronize()
            assert torch.equal(_raw(out), _raw(ref)), (h, w, matrix, full)
    lib = _lib.load()
    to_rgb, from_rgb = ops._f12(yuv.csc("bt601", False, depth)[0]), ops._f12(yuv.csc("bt601", False, out_depth)[1])
    f = _up(_frames(3, (B,) + yuv.frame_shape(H, W), depth, fmt), dev)
    o = torch.zeros((B,) + yuv.frame_shape(s * H, s * W), dtype=torch.int16, device=dev).view(torch.uint16)
    sb, db = ops._yuv_block(*ops.yuv420_views(f, fmt), "t"), ops._yuv_block(*ops.yuv420_views(o, fmt), "t")
    sm = int(fmt != "i420")
    call = lambda sb_, h, w, db_, sd=depth, dd=out_depth: lib.hat_plan_forward_yuv420_deep(p._h, *sb_, sd, sm, h, w, *db_, dd, sm, to_rgb, from_rgb, stream)
    bs = 1 if depth == 8 else 2
    assert call(sb, H, W, db) == 0
    assert call(sb[:1] + [bs * W - bs] + sb[2:], H, W, db) == -1                 # a Y row does not fit its pitch
    assert call(sb, H, W, db[:1] + [2 * s * W - 2] + db[2:]) == -1               # destination pitches
    assert call(sb, H, W, db[:5] + [db[6] * s * W // 2 - 2] + db[6:]) == -1
    assert call(sb, H, W, db[:1] + [db[1] + 1] + db[2:]) == -1                   # an odd pitch on a deep side
    assert call(sb, H // 2, W, db) == -1                                         # H - h >= h: no row to reflect
    assert call(sb, H + 2, W, db) == -1                                          # larger than the plan
    if fmt != "i420":
        assert call(sb, H, W, db, dd=8) == -1                                    # bytes there: an interleaved step of 4 is no byte layout
    if B > 1:                                                                    # samples overlap: refused before anything is enqueued
        assert call(sb, H, W, db[:2] + [db[1] * (s * H - 1)] + db[3:]) == -1
        assert call(sb, H, W, db[:7] + [db[5] * (s * H // 2 - 1)]) == -1
    torch.cuda.synchronize()
    p.close()


# ---------------------------------------------------------------------------------------------- 8
def test_frame_sequences_files_and_the_c_program(tmp_path):
    dev = _dev()
    from super_resolution_amd import frames as FR, plan, video
    net = _net("HAT", "hats_1g_x4", "bf16", dev)
    h, w = 38, 54
    seq = [_frames(100 + i, yuv.frame_shape(h, w), 10) for i in range(3)]
    want = [_down(net.forward_yuv420(_up(a, dev), fmt="i420", depth=10)[0]) for a in seq]
    want8 = [_down(net.forward_yuv420(_up(a, dev), fmt="i420", depth=10, out_depth=8)[0]) for a in seq]
    got = list(FR.upscale_frames(net, iter(seq), pixfmt="i420", depth=10))
    assert len(got) == 3
    for i in range(3):
        assert got[i].dtype == np.uint16 and got[i].shape == yuv.frame_shape(4 * h, 4 * w) and np.array_equal(got[i], want[i]), i
    with pytest.raises(RuntimeError, match="uint16"):
        next(FR.upscale_frames(net, iter([seq[0].astype(np.uint8)]), pixfmt="i420", depth=10))
    hdr = {"W": w, "H": h, "F": "25:1", "I": "p", "A": "1:1", "C": "420p10", "X": []}
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr, deep=True) as wr:
        for f in seq:
            wr.write(f)
    info = video.upscale_file(net, str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"))
    assert info["frames"] == 3 and info["out"] == (4 * w, 4 * h)
    with y4m.Reader(str(tmp_path / "out.y4m"), deep=True) as rd:
        assert rd.header == y4m.scaled_header(hdr, 4)
        assert all(np.array_equal(a, b) for a, b in zip(list(rd), want))
    args = video.parser().parse_args(["-opt", "o.yml", "-i", "a", "-o", "b", "--out-depth", "8"])
    video.upscale_file(net, str(tmp_path / "in.y4m"), str(tmp_path / "out8.y4m"), out_depth=args.out_depth)
    with y4m.Reader(str(tmp_path / "out8.y4m")) as rd:
        assert rd.header["C"] == "420"
        got8 = list(rd)
    assert len(got8) == 3 and all(np.array_equal(a, b) for a, b in zip(got8, want8))
    # the C example does the same from a plan (28 x 44 frames pad to the plan's 32 x 48)
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    exe = tmp_path / "plan_upscale_y4m"
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_y4m.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 32, 48), path)
    hs, wsz = 28, 44
    small = [_frames(80 + i, yuv.frame_shape(hs, wsz), 10) for i in range(3)]
    hdr2 = dict(hdr, W=wsz, H=hs)
    with y4m.Writer(str(tmp_path / "s.y4m"), hdr2, deep=True) as wr:
        for f in small:
            wr.write(f)
    for extra, od in (([], 10), (["8"], 8)):
        wants = [_down(net.forward_yuv420(_up(a, dev), fmt="i420", depth=10, out_depth=od)[0]) for a in small]
        r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, str(tmp_path / "s.y4m"), str(tmp_path / "c.y4m")] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        with y4m.Reader(str(tmp_path / "c.y4m"), deep=True) as rd:
            assert rd.header == y4m.with_depth(y4m.scaled_header(hdr2, 4), od)
            gotc = list(rd)
        assert len(gotc) == 3 and all(np.array_equal(a, b) for a, b in zip(gotc, wants)), od


# ---------------------------------------------------------------------------------------------- 9
def test_720p_headline_eight_to_ten_takes_the_fused_epilogue():
    dev = _dev()
    net = _net("HAT", HATS, "bf16", dev, upscale=4)
    eng = net.engine()
    h, w = 720, 1280
    frames = _frames(h + w, (1,) + yuv.frame_shape(h, w))
    x = torch.from_numpy(yuv.yuv420_to_planes(frames)).to(dev)
    out = torch.zeros((1,) + yuv.frame_shape(4 * h, 4 * w), dtype=torch.int16, device=dev).view(torch.uint16)
    d = torch.from_numpy(frames).to(dev)
    ref = yuv.planes_to_yuv420(net(x).cpu().numpy(), out_depth=10)
    net.forward_yuv420(d, out=out, out_depth=10)                 # (the workspace of this shape exists from the float forward)
    _raw(out).zero_()
    fused, planes = eng.yuv_fused_calls, eng.yuv_planes_calls
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    net.forward_yuv420(d, out=out, depth=8, out_depth=10)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (fused + 1, planes), "conv_last converts in its epilogue"
    assert np.array_equal(_down(out), ref)
    assert peak == 0, f"with out= nothing is allocated above the resident set, got {peak} bytes"
