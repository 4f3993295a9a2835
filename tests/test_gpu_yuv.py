"""The 4:2:0 frame boundary on the GPU: NV12 / NV21 / I420 frames in and out through the kernels, the engine, the modules, the
plans, the C example and the frame-sequence generator.  Every comparison is an equality against super_resolution_amd/yuv.py,
the numpy definition (tests/test_yuv_cpu.py pins that to the reference's colour conversion): every product and sum of the
conversion is rounded to fp32 on its own on both sides, so there is no tolerance and no share of pixels left out."""
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
MATRICES = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


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


def _frames(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _composition(net, frames, ws, s, dev, *, fmt="nv12", matrix="bt601", full_range=False):
    """host yuv420_to_planes (with the reflect-pad) -> this build's forward -> crop -> host planes_to_yuv420"""
    h, w = yuv.frame_size(frames.shape)
    pad = ((ws - h % ws) % ws, (ws - w % ws) % ws)
    x = yuv.yuv420_to_planes(frames, fmt=fmt, matrix=matrix, full_range=full_range, pad=pad)
    y = net(torch.from_numpy(x).to(dev)).cpu().numpy()
    return yuv.planes_to_yuv420(y, fmt=fmt, matrix=matrix, full_range=full_range, crop=(s * h, s * w))


def _pitched(B, h, w, fmt, dev, fill, y_extra=5, c_extra=3):
    """Device buffers for a (B, h, w) frame with a Y pitch of w + y_extra and a chroma pitch of the chroma row + c_extra bytes (odd
    for even rows: never a multiple of 4); returns the buffers and the views y, cb, cr."""
    ybuf = torch.full((B, h, w + y_extra), fill, dtype=torch.uint8, device=dev)
    if fmt == "i420":
        cbuf = torch.full((2, B, h // 2, w // 2 + c_extra), fill, dtype=torch.uint8, device=dev)
        cb, cr = cbuf[0, :, :, :w // 2], cbuf[1, :, :, :w // 2]
    else:
        cbuf = torch.full((B, h // 2, w + c_extra), fill, dtype=torch.uint8, device=dev)
        a, b = cbuf[:, :, 0:w:2], cbuf[:, :, 1:w:2]
        cb, cr = (a, b) if fmt == "nv12" else (b, a)
    return ybuf, cbuf, (ybuf[:, :, :w], cb, cr)


def _guards_intact(ybuf, cbuf, w, fmt, fill):
    if not bool((ybuf[:, :, w:] == fill).all()):
        return False
    return bool((cbuf[..., (w // 2 if fmt == "i420" else w):] == fill).all())


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("pad", [(0, 0), (6, 0), (0, 6), (6, 6)])
def test_yuv420_to_planes_is_the_definition(pad, fmt):
    dev = _dev()
    from super_resolution_amd import ops
    B, h, w = 2, 38, 302                                        # not multiples of the 256-pixel workgroup row
    Y, Cb, Cr = _frames(1, (B, h, w)), _frames(2, (B, h // 2, w // 2)), _frames(3, (B, h // 2, w // 2))
    for a in (Y, Cb, Cr):
        a.reshape(-1)[-256:] = np.arange(256, dtype=np.uint8)    # every byte value is present
    Y[0, 0, 0:2], Cb[0, 0, 0], Cr[0, 0, 0] = 16, 128, 16         # drives G above nothing, R below 0
    Y[0, 0, 2:4], Cb[0, 0, 1], Cr[0, 0, 1] = 235, 128, 240       # drives R above 1
    frame = yuv.join(Y, Cb, Cr, fmt)
    ybuf, cbuf, (y, cb, cr) = _pitched(B, h, w, fmt, dev, 0)
    y.copy_(torch.from_numpy(Y)), cb.copy_(torch.from_numpy(Cb)), cr.copy_(torch.from_numpy(Cr))
    assert y.stride(1) == w + 5 and cb.stride(1) % 4 != 0 and cb.stride(2) == (1 if fmt == "i420" else 2)
    Hp, Wp = h + pad[0], w + pad[1]
    big = torch.full((B * 3 * Hp * Wp + 64,), -7.0, device=dev)
    dst = big[32:-32].view(B, 3, Hp, Wp)
    for matrix, full in MATRICES:
        to_rgb, _ = yuv.csc(matrix, full)
        ops.yuv420_to_planes(y, cb, cr, dst, to_rgb)
        torch.cuda.synchronize()
        ref = yuv.yuv420_to_planes(frame, fmt=fmt, matrix=matrix, full_range=full, pad=pad)
        assert ref[0, 0, 0, 0] == 0.0 and ref[0, 0, 0, 2] == 1.0, "the two triples are clamped"
        assert np.array_equal(dst.cpu().numpy(), ref), (matrix, full)
    assert bool((big[:32] == -7.0).all()) and bool((big[-32:] == -7.0).all()), "floats outside the planes are not the kernel's"


# ---------------------------------------------------------------------------------------------- 2
def _special_planes(B, Hs, Ws):
    """Zeros of both signs, 1 and its successor, the infinities, every k / 255, every half-way point between two 8-bit levels
    with its fp32 neighbours, and uniform values in [-0.5, 1.5)."""
    g = torch.Generator().manual_seed(5)
    t = torch.rand(B * 3 * Hs * Ws, generator=g) * 2.0 - 0.5
    k = torch.arange(256, dtype=torch.float32)
    half = (k[:255] + 0.5) / 255.0
    up, down = torch.nextafter(half, torch.tensor(2.0)), torch.nextafter(half, torch.tensor(-1.0))
    one = torch.tensor(1.0)
    sp = torch.cat([torch.tensor([-0.0, 0.0, 1.0, float(torch.nextafter(one, torch.tensor(2.0))), float("inf"), float("-inf")]),
                    k / 255.0, half, up, down, torch.nextafter(up, torch.tensor(2.0)), torch.nextafter(down, torch.tensor(-1.0))])
    assert sp.numel() <= Hs * Ws
    t = t.reshape(B, 3, Hs * Ws)
    for c in range(3):                                           # each plane carries them, shifted so that they meet different partners
        t[0, c, 100 * c:100 * c + sp.numel()] = sp
    return t.reshape(B, 3, Hs, Ws)


@pytest.fixture(scope="module")
def special():
    return _special_planes(2, 31, 61)


@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("crop", [(30, 60), (26, 56), (30, 50)])
def test_planes_to_yuv420_is_the_definition(crop, fmt, special):
    dev = _dev()
    from super_resolution_amd import ops
    B, (ho, wo) = 2, crop
    src = special.to(dev)
    for matrix, full in MATRICES:
        _, from_rgb = yuv.csc(matrix, full)
        ref = yuv.planes_to_yuv420(special.numpy(), fmt=fmt, matrix=matrix, full_range=full, crop=crop)
        ybuf, cbuf, (y, cb, cr) = _pitched(B, ho, wo, fmt, dev, 99)       # odd pitches: single-byte stores
        ops.planes_to_yuv420(src, y, cb, cr, from_rgb)
        packed = torch.full((B,) + yuv.frame_shape(ho, wo), 99, dtype=torch.uint8, device=dev)   # the standard layout: dword Y stores
        ops.planes_to_yuv420(src, *ops.yuv420_views(packed, fmt), from_rgb)
        torch.cuda.synchronize()
        got = yuv.join(y.cpu().numpy(), cb.cpu().numpy(), cr.cpu().numpy(), fmt)
        assert np.array_equal(got, ref), (matrix, full)
        assert np.array_equal(packed.cpu().numpy(), ref), (matrix, full)
        assert _guards_intact(ybuf, cbuf, wo, fmt, 99), "bytes between the rows are not the kernel's"


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("shape", [(24, 16), (24, 48), (72, 5120)], ids=["24x16", "24x48", "72x5120"])
def test_conv3x3_to_yuv420_equals_planes_then_convert(shape):
    """24 rows: three 8-row bands, so the carried row pair crosses the three-row unroll; 48 columns: several strips; 72 x 5120:
    the planes geometry has 9 rows per band there, so the round-up to an even band height is exercised."""
    dev = _dev()
    from super_resolution_amd import _lib, ops
    from super_resolution_amd.engine import RGB_MEAN
    import ctypes as C
    H, W = shape
    rows, units = C.c_int32(0), C.c_int32(0)
    B = 2
    g = torch.Generator().manual_seed(W)
    x = (torch.randn(B, H, W, 64, generator=g)).to(torch.bfloat16).to(dev)
    wl = torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0)    # outputs spread over and beyond [0, 1] around the mean
    bl = torch.randn(3, generator=g) * 0.1
    wpk, b8 = ops.pack_cab_squeeze(wl, bl, dev)
    kw = dict(B=B, H=H, W=W, C_=64, ldx=64, out_scale=0.5, mean=RGB_MEAN, dtype=ops.HAT_BF16)
    planes = torch.empty(B, 3, H, W, device=dev)
    ops.conv3x3_to_planes(x, wpk, b8, planes, n_out=3, **kw)
    torch.cuda.synchronize()
    inside = float(((planes > 0) & (planes < 1)).float().mean())
    assert 0.3 < inside < 0.95, inside                           # neither all saturated nor all interior
    if W == 5120:
        strips = (W + 13) // 14
        assert -(-H // (3072 // strips)) == 9, "the planes geometry has an odd band height here"
    _, from_rgb = yuv.csc("bt601", False)
    _, from_709 = yuv.csc("bt709", True)
    for ho, wo in ((H, W), (H - 4, W - 6), (H - 2, (W // 14) * 14 if W > 16 else 14), (2, 2)):
        for fmt, m in (("nv12", from_rgb), ("i420", from_709)):
            ref = torch.empty((B,) + yuv.frame_shape(ho, wo), dtype=torch.uint8, device=dev)
            ops.planes_to_yuv420(planes, *ops.yuv420_views(ref, fmt), m)
            ybuf, cbuf, (y, cb, cr) = _pitched(B, ho, wo, fmt, dev, 77, y_extra=1, c_extra=1)
            ops.conv3x3_to_yuv420(x, wpk, b8, y, cb, cr, from_rgb=m, **kw)
            torch.cuda.synchronize()
            ry, rcb, rcr = ops.yuv420_views(ref, fmt)
            assert torch.equal(y, ry), (ho, wo, fmt, "Y")
            assert torch.equal(cb, rcb) and torch.equal(cr, rcr), (ho, wo, fmt, "chroma")
            assert _guards_intact(ybuf, cbuf, wo, fmt, 77)
    ref8 = torch.empty(B, H - 3, W - 5, 3, dtype=torch.uint8, device=dev)      # the u8 and planes routes are what they were
    ops.planes_to_u8(planes, ref8)
    out8 = torch.empty_like(ref8)
    ops.conv3x3_to_u8(x, wpk, b8, out8, h_out=H - 3, w_out=W - 5, bgr=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out8, ref8)


# ---------------------------------------------------------------------------------------------- 4, 10
CASES = [("HAT", "tiny_x2", (1, 38, 54), "nv12", ("bt601", False)), ("HAT", "tiny_x4", (2, 38, 54), "i420", ("bt709", False)),
         ("HAT", "tiny_x3", (1, 16, 10), "nv21", ("bt601", True)), ("HATX", "hatx_tiny_plain_x2", (2, 38, 54), "nv12", ("bt709", True))]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[1]}_B{c[2][0]}_{c[2][1]}x{c[2][2]}_{c[3]}" for c in CASES])
def test_forward_yuv420_is_the_composition(case, dtype):
    dev = _dev()
    arch, name, (B, h, w), fmt, (matrix, full) = case
    cfg = META["cfgs"][name]
    ws, s = cfg["window_size"], cfg["upscale"]
    net = _net(arch, name, dtype, dev)
    frames = _frames(h * w + B, (B,) + yuv.frame_shape(h, w))
    kw = dict(fmt=fmt, matrix=matrix, full_range=full)
    ref = _composition(net, frames, ws, s, dev, **kw)
    d = torch.from_numpy(frames).to(dev)
    eng = net.engine()
    counts = (eng.yuv_fused_calls, eng.yuv_planes_calls)
    out = net.forward_yuv420(d, **kw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B,) + yuv.frame_shape(s * h, s * w)
    assert np.array_equal(out.cpu().numpy(), ref)
    fused = dtype == "bf16" and (s * -(-w // ws) * ws) % 16 == 0
    assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (counts[0] + int(fused), counts[1] + int(not fused))
    if B == 1:                                                   # (3h/2, w) is accepted as one frame
        assert np.array_equal(net.forward_yuv420(d[0], **kw).cpu().numpy(), ref)
    mine = torch.zeros_like(out)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    got = net.forward_yuv420(d, out=mine, **kw)
    torch.cuda.synchronize()
    assert got is mine and np.array_equal(mine.cpu().numpy(), ref), "out= is filled with the same bytes"
    assert torch.cuda.memory_allocated(dev) == before, "with out= the call keeps nothing"
    if fused:
        assert torch.cuda.max_memory_allocated(dev) == before, "with out= and the fused epilogue the call allocates nothing"


def test_forward_yuv420_is_deterministic():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "bf16", dev)
    d = torch.from_numpy(_frames(77, (2,) + yuv.frame_shape(38, 54))).to(dev)
    a = net.forward_yuv420(d, fmt="i420")
    b = net.forward_yuv420(d, fmt="i420")
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()


# ---------------------------------------------------------------------------------------------- 5
def test_forward_yuv420_refusals():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "f32", dev)
    z = lambda *shape, **kw: torch.zeros(*shape, dtype=torch.uint8, device=dev, **kw)
    with pytest.raises(RuntimeError, match="even"):
        net.forward_yuv420(z(1, 24, 21))                         # odd w
    with pytest.raises(RuntimeError, match="even"):
        net.forward_yuv420(z(1, 25, 20))                         # 25 rows are not 3h/2 for an even h (an odd h has no such array)
    with pytest.raises(TypeError, match="uint8"):
        net.forward_yuv420(torch.zeros(1, 24, 20, device=dev))
    with pytest.raises(RuntimeError, match="GPU"):
        net.forward_yuv420(torch.zeros(1, 24, 20, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="format"):
        net.forward_yuv420(z(1, 24, 20), fmt="yuyv")
    with pytest.raises(RuntimeError, match="matrix"):
        net.forward_yuv420(z(1, 24, 20), matrix="bt2020")
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv420(z(1, 24, 20), out=z(1, 48, 41))
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv420(z(1, 24, 20), out=torch.zeros(1, 48, 40, device=dev))
    with pytest.raises(RuntimeError, match="reflect"):
        net.forward_yuv420(z(1, 6, 20))                          # 4 rows cannot be padded to 8
    net1 = _net("HAT", "tiny_x2", "f32", dev, in_chans=1)
    with pytest.raises(RuntimeError, match="in_chans"):
        net1.forward_yuv420(z(1, 24, 16))


# ---------------------------------------------------------------------------------------------- 6
def test_720p_headline_takes_the_fused_epilogue_and_never_holds_the_float_image():
    dev = _dev()
    net = _net("HAT", HATS, "bf16", dev, upscale=4)
    eng = net.engine()
    image_bytes = 3 * 2880 * 5120 * 4
    h, w = 720, 1280
    frames = _frames(h + w, (1,) + yuv.frame_shape(h, w))
    x = torch.from_numpy(yuv.yuv420_to_planes(frames)).to(dev)
    out = torch.zeros((1,) + yuv.frame_shape(4 * h, 4 * w), dtype=torch.uint8, device=dev)   # the caller's result tensor, as a frame loop holds it
    d = torch.from_numpy(frames).to(dev)
    net.forward_yuv420(d, out=out)                               # the first call builds the workspace of this shape
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    y = net(x)
    torch.cuda.synchronize()
    peak_f = torch.cuda.max_memory_allocated(dev) - base
    ref = yuv.planes_to_yuv420(y.cpu().numpy())
    del y
    out.zero_()
    fused, planes = eng.yuv_fused_calls, eng.yuv_planes_calls
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    net.forward_yuv420(d, out=out)
    torch.cuda.synchronize()
    peak_y = torch.cuda.max_memory_allocated(dev) - base
    assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (fused + 1, planes), "conv_last converts in its epilogue"
    assert np.array_equal(out.cpu().numpy(), ref)
    print(f"peak above the resident set: forward {peak_f / 1e6:.1f} MB, forward_yuv420 {peak_y / 1e6:.1f} MB")
    assert peak_y <= peak_f - image_bytes, (peak_f, peak_y)      # the fp32 image is never allocated


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case", [("HAT", "hats_1g_x4", "bf16", (1, 3, 32, 48), (28, 42), "nv12"), ("HATX", "hatx_tiny_plain_x2", "f32", (2, 3, 16, 24), (14, 20), "i420")],
                         ids=["hats_bf16", "hatx_f32_B2"])
def test_plan_forward_yuv420(case, tmp_path):
    dev = _dev()
    from super_resolution_amd import _lib, ops, plan
    arch, name, dtype, shape, small, fmt = case
    B, _, H, W = shape
    s = META["cfgs"][name]["upscale"]
    net = _net(arch, name, dtype, dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, shape, path)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    for h, w in ((H, W), small):                                 # the smaller frame pads to the plan's shape, as forward_yuv420 pads it
        frames = torch.from_numpy(_frames(h + w, (B,) + yuv.frame_shape(h, w))).to(dev)
        for matrix, full in (("bt601", False), ("bt709", True)):
            ref = net.forward_yuv420(frames, fmt=fmt, matrix=matrix, full_range=full)
            out = torch.full((B,) + yuv.frame_shape(s * h, s * w), 9, dtype=torch.uint8, device=dev)
            p.forward_yuv420(frames, out, fmt=fmt, matrix=matrix, full_range=full, stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (h, w, matrix, full)
    lib = _lib.load()
    to_rgb, from_rgb = (ops._f12(m) for m in yuv.csc())
    f = torch.from_numpy(_frames(3, (B,) + yuv.frame_shape(H, W))).to(dev)
    o = torch.zeros((B,) + yuv.frame_shape(s * H, s * W), dtype=torch.uint8, device=dev)
    sb, db = ops._yuv_block(*ops.yuv420_views(f, fmt), "t"), ops._yuv_block(*ops.yuv420_views(o, fmt), "t")
    call = lambda sb_, h, w, db_: lib.hat_plan_forward_yuv420(p._h, *sb_, h, w, *db_, to_rgb, from_rgb, stream)
    step = sb[6]
    assert call(sb, H, W, db) == 0
    assert call(sb[:1] + [W - 1] + sb[2:], H, W, db) == -1                      # a Y row does not fit its pitch
    assert call(sb[:5] + [step * W // 2 - 1] + sb[6:], H, W, db) == -1          # a chroma row does not fit its pitch
    assert call(sb, H, W, db[:1] + [s * W - 1] + db[2:]) == -1                  # destination pitches
    assert call(sb, H, W, db[:5] + [step * s * W // 2 - 1] + db[6:]) == -1
    assert call(sb, H // 2, W, db) == -1                                         # H - h >= h: no row to reflect
    assert call(sb, H + 2, W, db) == -1                                          # larger than the plan
    if B > 1:                                                                    # samples overlap: refused before anything is enqueued
        assert call(sb[:2] + [sb[1] * (H - 1) + W - 1] + sb[3:], H, W, db) == -1 and call(sb, H, W, db[:2] + [db[1] * (s * H - 1)] + db[3:]) == -1
        assert call(sb, H, W, db[:7] + [db[5] * (s * H // 2 - 1)]) == -1
    torch.cuda.synchronize()
    p.close()


# ---------------------------------------------------------------------------------------------- 8
def test_c_program_upscales_a_y4m(tmp_path):
    dev = _dev()
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from super_resolution_amd import plan
    exe = tmp_path / "plan_upscale_y4m"
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_y4m.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    net = _net("HAT", "hats_1g_x4", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 32, 48), path)
    h, w = 28, 44
    frames = [_frames(80 + i, yuv.frame_shape(h, w)) for i in range(3)]
    hdr = {"W": w, "H": h, "F": "25:1", "I": "p", "A": "1:1", "C": "420jpeg", "X": []}
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr) as wr:
        for f in frames:
            wr.write(f)
    want = [net.forward_yuv420(torch.from_numpy(f).to(dev), fmt="i420")[0].cpu().numpy() for f in frames]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with y4m.Reader(str(tmp_path / "out.y4m")) as rd:
        assert rd.header == y4m.scaled_header(hdr, 4)
        got = list(rd)
    assert len(got) == 3
    for i in range(3):
        assert np.array_equal(got[i], want[i]), f"frame {i}"


# ---------------------------------------------------------------------------------------------- 9
def test_upscale_frames_420_matches_forward_yuv420_in_order():
    dev = _dev()
    from super_resolution_amd import frames as FR
    net = _net("HAT", dict(HATS, depths=[2], num_heads=[6]), "bf16", dev, upscale=2)
    h, w = 46, 70
    seq = [_frames(100 + i, yuv.frame_shape(h, w)) for i in range(5)]
    assert len({a.tobytes() for a in seq}) == 5
    for pixfmt, kw in (("i420", {}), ("nv12", dict(matrix="bt709", full_range=True))):
        want = [net.forward_yuv420(torch.from_numpy(a).to(dev), fmt=pixfmt, **kw)[0].cpu().numpy() for a in seq]
        got = list(FR.upscale_frames(net, iter(seq), pixfmt=pixfmt, **kw))
        assert len(got) == 5
        for i in range(5):
            assert got[i].dtype == np.uint8 and got[i].shape == yuv.frame_shape(2 * h, 2 * w) and np.array_equal(got[i], want[i]), (pixfmt, i)
    one = list(FR.upscale_frames(net, seq[:1], pixfmt="nv12", **kw))
    assert len(one) == 1 and np.array_equal(one[0], want[0])
    assert list(FR.upscale_frames(net, [], pixfmt="i420")) == []
    side = torch.cuda.Stream(device=dev)                          # the caller switches stream between frames
    gen, got2 = FR.upscale_frames(net, iter(seq[:4]), pixfmt="nv12", **kw), []
    for i in range(4):
        if i % 2:
            with torch.cuda.stream(side):
                got2.append(next(gen))
        else:
            got2.append(next(gen))
    assert next(gen, None) is None
    for i in range(4):
        assert np.array_equal(got2[i], want[i]), f"frame {i} with a switched stream"
    rgb = [_frames(200 + i, (45, 70, 3)) for i in range(3)]       # the default is what it was
    got3 = list(FR.upscale_frames(net, iter(rgb), pixfmt="rgb24"))
    for a, b in zip(rgb, got3):
        assert np.array_equal(b, net.forward_u8(torch.from_numpy(a).to(dev))[0].cpu().numpy())
    with pytest.raises(RuntimeError, match="pixfmt"):
        next(FR.upscale_frames(net, iter(seq), pixfmt="yuyv"))
    with pytest.raises(RuntimeError, match="uint8"):
        next(FR.upscale_frames(net, iter(rgb), pixfmt="i420"))
