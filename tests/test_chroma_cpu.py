"""4:2:2, 4:4:4 and grey on the host: the general definition of super_resolution_amd/yuv.py (yuv_to_planes / planes_to_yuv and the
layout functions), the Y4M colour spaces behind chroma=True, the HatYuvSurface layout and the refusals of the surface entries,
which need no GPU.  Every comparison of two definitions is array_equal."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from helpers import golden
from super_resolution_amd import y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("i422", "nv16", "i444", "nv24", "gray")


def _frame(seed, h, w, fmt, depth=8, msb=None):
    dt, _, maxcode, shift = yuv.container(depth, fmt, msb)
    rng = np.random.default_rng(seed)
    return (rng.integers(0, maxcode + 1, (2,) + yuv.frame_shape_fmt(h, w, fmt)).astype(np.uint16) << shift).astype(dt)


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("msb", [True, False])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_general_definition_is_the_420_definition(fmt, depth, msb):
    frame = _frame(1, 12, 10, fmt, depth, msb)
    for pad in ((0, 0), (5, 3)):
        for matrix, full in (("bt601", False), ("bt709", True)):
            kw = dict(fmt=fmt, matrix=matrix, full_range=full, depth=depth, msb=msb)
            assert np.array_equal(yuv.yuv_to_planes(frame, pad=pad, **kw), yuv.yuv420_to_planes(frame, pad=pad, **kw))
    rng = np.random.default_rng(2)
    planes = (rng.random((2, 3, 11, 13), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    planes[0, :, 0, :3] = [np.inf, -np.inf, -0.0]
    for crop in (None, (10, 12), (2, 2)):
        if crop is None:
            p, crop = planes[:, :, :10, :12], None
        else:
            p = planes
        kw = dict(fmt=fmt, matrix="bt709", out_depth=depth, msb=msb, crop=crop)
        assert np.array_equal(yuv.planes_to_yuv(p, **kw), yuv.planes_to_yuv420(p, **kw))
    assert yuv.frame_shape_fmt(12, 10, fmt) == yuv.frame_shape(12, 10) and yuv.frame_size_fmt((18, 10), fmt) == yuv.frame_size((18, 10))
    for a, b in zip(yuv.split_fmt(frame, fmt), yuv.split(frame, fmt)):
        assert np.array_equal(a, b)


def test_444_is_the_reference_conversion():
    """4:4:4 has no subsampling, so the general path must reproduce the reference's per-pixel conversion, which
    tests/golden/ycbcr_bt601.npz holds (basicsr's color_util on a grid of triples).  Input side: an i444 frame of the golden's
    triples through yuv_to_planes against the reference's RGB, 2e-6 in [0, 1] units (the bar test_yuv_cpu.py pins ycc_to_rgb
    with).  Output side: the un-rounded Y, cb + k, cr + k of the general path's per-pixel expression against the reference's
    YCbCr in ITS units ([0, 1]: byte units / 255), the same 2e-6; and the bytes planes_to_yuv(fmt='i444') stores are those values
    rounded half to even, exactly."""
    g = golden("ycbcr_bt601.npz")
    ycc, ref = g["ycc"], g["rgb_ref"]
    n = ycc.shape[0]
    frame = yuv.join_fmt(ycc[:, 0].reshape(1, n), ycc[:, 1].reshape(1, n), ycc[:, 2].reshape(1, n), "i444")
    assert frame.shape == (3, n)
    got = yuv.yuv_to_planes(frame, fmt="i444")[0, :, 0, :].T
    assert float(np.abs(got.astype(np.float64) - np.clip(ref, 0, 1)).max()) <= 2e-6
    rgb, ref2 = g["rgb"], g["ycc_ref"]
    _, k = yuv.csc("bt601", False)
    planes = np.ascontiguousarray(rgb.T.reshape(1, 3, 1, -1))
    Y, cb, cr = yuv.rgb_to_ycc_float(planes, k)
    pre = np.stack([Y[0, 0], cb[0, 0] + k[7], cr[0, 0] + k[11]], axis=1)
    assert pre.dtype == np.float32
    assert float(np.abs(pre.astype(np.float64) / 255.0 - ref2.astype(np.float64)).max()) <= 2e-6
    out = yuv.planes_to_yuv(planes, fmt="i444")
    Yb, Cbb, Crb = yuv.split_fmt(out, "i444")
    want = np.rint(np.clip(pre, 0, 255)).astype(np.uint8)
    assert np.array_equal(np.stack([Yb[0, 0], Cbb[0, 0], Crb[0, 0]], axis=1), want)
    # nv24 holds the same samples interleaved; gray holds Y alone
    assert np.array_equal(np.stack(yuv.split_fmt(yuv.planes_to_yuv(planes, fmt="nv24"), "nv24"))[:, 0, 0].T, want)
    assert np.array_equal(yuv.planes_to_yuv(planes, fmt="gray")[0, 0], want[:, 0])


def test_422_and_grey_expressions():
    rng = np.random.default_rng(3)
    planes = rng.random((1, 3, 5, 6), dtype=np.float32)
    _, k = yuv.csc("bt709", True, 10)
    Y, cb, cr = yuv.rgb_to_ycc_float(planes, k)
    want_cb = (cb[:, :, 0::2] + cb[:, :, 1::2]) * np.float32(0.5) + k[7]
    want_cr = (cr[:, :, 0::2] + cr[:, :, 1::2]) * np.float32(0.5) + k[11]
    for fmt in ("i422", "nv16"):
        out = yuv.planes_to_yuv(planes, fmt=fmt, matrix="bt709", full_range=True, out_depth=10)
        Yc, Cbc, Crc = (yuv.decode(a, 10, fmt) for a in yuv.split_fmt(out, fmt))
        q = lambda v: np.rint(np.clip(v * np.float32(4.0), 0, 1023)).astype(np.uint16)
        assert np.array_equal(Yc, q(Y)) and np.array_equal(Cbc, q(want_cb)) and np.array_equal(Crc, q(want_cr))
    # grey in: Cb' = Cr' = 0 exactly, i.e. the i444 frame whose chroma planes hold the neutral code
    for depth in (8, 10, 16):
        gfr = _frame(4, 5, 7, "gray", depth)
        neutral = np.full_like(gfr, 128 << (depth - 8))
        full = yuv.join_fmt(gfr, neutral, neutral, "i444", depth)
        assert np.array_equal(yuv.yuv_to_planes(gfr, fmt="gray", depth=depth, pad=(2, 3)), yuv.yuv_to_planes(full, fmt="i444", depth=depth, pad=(2, 3)))
    # nearest chroma: every pixel of a 4:2:2 pair reads the pair's sample
    fr = _frame(5, 3, 6, "i422")
    Yv, Cbv, Crv = yuv.split_fmt(fr, "i422")
    up = yuv.join_fmt(Yv, np.repeat(Cbv, 2, axis=-1), np.repeat(Crv, 2, axis=-1), "i444")
    assert np.array_equal(yuv.yuv_to_planes(fr, fmt="i422", pad=(1, 4)), yuv.yuv_to_planes(up, fmt="i444", pad=(1, 4)))


@pytest.mark.parametrize("depth", yuv.DEPTHS)
@pytest.mark.parametrize("fmt", yuv.ALL_FORMATS)
def test_layouts_round_trip(fmt, depth):
    sub_x, sub_y, kind = yuv.LAYOUTS[fmt]
    h, w = (6 if sub_y == 1 else 5), (8 if sub_x == 1 else 7)
    shape = yuv.frame_shape_fmt(h, w, fmt)
    assert shape == ({"gray": h, "i444": 3 * h, "nv24": 3 * h, "i422": 2 * h, "nv16": 2 * h}.get(fmt, 3 * h // 2), w)
    assert yuv.frame_size_fmt((2,) + shape, fmt) == (h, w)
    dt = yuv.container(depth, fmt)[0]
    frame = np.arange(2 * shape[0] * shape[1]).reshape((2,) + shape).astype(dt)
    Y, Cb, Cr = yuv.split_fmt(frame, fmt, depth)
    assert Y.shape == (2, h, w) and np.shares_memory(Y, frame)
    if kind == "gray":
        assert Cb is None and Cr is None
    else:
        assert Cb.shape == Cr.shape == (2, h >> sub_y, w >> sub_x) and np.shares_memory(Cb, frame)
        first = frame[0, h].reshape(-1)
        assert Cb[0, 0, 0] == first[1 if kind == "semi_vu" else 0]
        assert Cr[0, 0, 0] == (first[0] if kind == "semi_vu" else first[1] if kind == "semi" else frame[0, h:].reshape(-1)[Cb[0].size])
    assert np.array_equal(yuv.join_fmt(Y, Cb, Cr, fmt, depth), frame)
    assert bool(yuv.container(10, fmt)[3]) == (kind in ("semi", "semi_vu")), "deep default: MSB for interleaved chroma, LSB for planes"


def test_size_refusals_by_name():
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    with pytest.raises(RuntimeError, match="i422.*even width"):
        yuv.yuv_to_planes(z(8, 5), fmt="i422")
    with pytest.raises(RuntimeError, match="nv16.*even width"):
        yuv.planes_to_yuv(np.zeros((1, 3, 8, 8), dtype=np.float32), fmt="nv16", crop=(3, 5))
    with pytest.raises(RuntimeError, match="i420.*even height"):
        yuv.planes_to_yuv(np.zeros((1, 3, 8, 8), dtype=np.float32), fmt="i420", crop=(3, 4))
    with pytest.raises(RuntimeError, match="nv12.*even height"):
        yuv.frame_shape_fmt(5, 4, "nv12")
    with pytest.raises(RuntimeError, match="smaller"):
        yuv.yuv_to_planes(z(9, 5), fmt="i444", pad=(3, 0))       # h = 3
    with pytest.raises(RuntimeError, match="smaller"):
        yuv.yuv_to_planes(z(3, 5), fmt="gray", pad=(0, 5))
    with pytest.raises(RuntimeError, match="format"):
        yuv.yuv_to_planes(z(6, 4), fmt="yuyv")
    with pytest.raises(RuntimeError, match="3h"):
        yuv.frame_size_fmt((7, 4), "i444")
    assert yuv.yuv_to_planes(z(3, 1), fmt="i444").shape == (1, 3, 1, 1), "a single pixel is a 4:4:4 frame"
    assert yuv.planes_to_yuv(np.zeros((1, 3, 4, 4), dtype=np.float32), fmt="gray", crop=(1, 3)).shape == (1, 1, 3)
    assert yuv.FORMATS == ("nv12", "nv21", "i420") and set(yuv.ALL_FORMATS) == set(yuv.FORMATS) | set(NEW)


# ---------------------------------------------------------------------------------------------- Y4M
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("c", ["422", "444", "mono"])
def test_y4m_round_trip(c, bits):
    fmt = y4m.CHROMAS[c]
    w, h = (6, 3) if c == "422" else (5, 3)
    hdr = y4m.with_chroma({"W": w, "H": h, "F": "30000:1001", "I": "p", "A": "1:1", "X": ["YSCSS=x"]}, c, bits)
    assert hdr["C"] == (c if bits == 8 else (f"mono{bits}" if c == "mono" else f"{c}p{bits}"))
    assert y4m.chroma(hdr) == c and y4m.depth(hdr) == bits
    frames = [_frame(10 + i, h, w, fmt, bits, False)[0] for i in range(3)]
    f = io.BytesIO()
    with y4m.Writer(f, hdr, chroma=True) as wr:
        assert wr.fmt == fmt
        for a in frames:
            wr.write(a)
        with pytest.raises(y4m.Y4MError, match="frame"):
            wr.write(np.zeros((h + 1, w), dtype=frames[0].dtype))
        raw = f.getvalue()
    n = frames[0].size * frames[0].itemsize
    assert len(raw) == len(y4m.format_header(hdr, chroma=True)) + 3 * (6 + n), "the record sizes follow the subsampling"
    rd = y4m.Reader(io.BytesIO(raw), chroma=True)
    assert rd.header == hdr and rd.fmt == fmt and rd.depth == bits and (rd.w, rd.h) == (w, h)
    got = list(rd)
    assert len(got) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, frames))
    assert got[0].shape == yuv.frame_shape_fmt(h, w, fmt)
    assert y4m.with_chroma(hdr, c) == hdr and y4m.chroma(y4m.with_chroma(hdr, "420")) == "420"
    assert y4m.with_depth(hdr, 8)["C"] == c, "with_depth keeps the subsampling"


def test_y4m_refusals():
    p = lambda s, **kw: y4m.parse_header(b"YUV4MPEG2 W4 H4 " + s, **kw)
    with pytest.raises(y4m.Y4MError, match="C444alpha"):
        p(b"C444alpha", chroma=True)
    with pytest.raises(y4m.Y4MError, match="C411"):
        p(b"C411", chroma=True)
    with pytest.raises(y4m.Y4MError, match="C422p14"):
        p(b"C422p14", chroma=True)
    with pytest.raises(y4m.Y4MError, match="Cmonop10"):
        p(b"Cmonop10", chroma=True)
    with pytest.raises(y4m.Y4MError, match="even width.*W5"):
        y4m.parse_header(b"YUV4MPEG2 W5 H4 C422", chroma=True)
    with pytest.raises(y4m.Y4MError, match="even.*H3"):
        y4m.parse_header(b"YUV4MPEG2 W4 H3 C420jpeg", chroma=True)
    assert y4m.parse_header(b"YUV4MPEG2 W5 H3 C444", chroma=True)["C"] == "444"
    assert y4m.parse_header(b"YUV4MPEG2 W4 H4 C420p10", chroma=True)["C"] == "420p10", "chroma=True includes deep=True"
    with pytest.raises(y4m.Y4MError, match="unknown chroma"):
        y4m.with_chroma({"W": 4, "H": 4}, "411")
    # without the keyword: the refusals and the messages that were
    with pytest.raises(y4m.Y4MError, match=r"colour space C444 is not supported: only 8-bit 4:2:0 \(C420, C420jpeg, C420mpeg2, C420paldv\)"):
        p(b"C444")
    with pytest.raises(y4m.Y4MError, match=r"colour space C422 is not supported: only 8-bit 4:2:0"):
        y4m.Writer(io.BytesIO(), {"W": 4, "H": 2, "C": "422"})
    with pytest.raises(y4m.Y4MError, match=r"colour space Cmono is not supported: only 8-bit 4:2:0"):
        y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H4 Cmono\n"))
    with pytest.raises(y4m.Y4MError, match=r"colour space C444p10 is not supported: only 8-bit 4:2:0"):
        p(b"C444p10", deep=True)
    with pytest.raises(y4m.Y4MError, match="colour space C420p10 has more than 8 bits per sample: only 8-bit 4:2:0 is supported"):
        p(b"C420p10")
    assert y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H4\n")).fmt == "i420"


def test_video_parser_takes_out_chroma():
    from super_resolution_amd import video
    base = ["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m"]
    assert video.parser().parse_args(base).out_chroma is None
    for c in ("420", "422", "444", "mono"):
        assert video.parser().parse_args(base + ["--out-chroma", c]).out_chroma == c
    with pytest.raises(SystemExit):
        video.parser().parse_args(base + ["--out-chroma", "411"])


# ---------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_surface_layout_matches_c(lib, tmp_path):
    """Compile a tiny C program against the header and compare sizeof / offsetof with ctypes."""
    from super_resolution_amd import _lib
    S = _lib.HatYuvSurface
    fields = [f[0] for f in S._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hat_mi355x.h"\nint main(){printf("%zu", sizeof(HatYuvSurface));\n'
    prog += "".join(f'printf(" %zu", offsetof(HatYuvSurface, {f}));\n' for f in fields) + "return 0;}\n"
    src = tmp_path / "layout.c"
    src.write_text(prog)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(S)
    assert vals[1:] == [getattr(S, f).offset for f in fields]


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    for name in ("hat_yuv_to_planes", "hat_planes_to_yuv", "hat_conv3x3_to_yuv", "hat_plan_forward_yuv"):
        assert getattr(lib, name) is not None
    assert lib.hat_abi_version() == 2
    text = open(os.path.join(ROOT, "include", "hat_mi355x.h")).read()
    for name in ("HatYuvSurface", "hat_yuv_to_planes(", "hat_planes_to_yuv(", "hat_conv3x3_to_yuv(", "hat_plan_forward_yuv("):
        assert name in text


def _surf(**kw):
    """A good 8-bit 4:2:2 planar surface of a (2, 6, 8) block at made-up (never dereferenced) addresses, then the changes."""
    from super_resolution_amd import _lib
    d = dict(y=0x10000, y_pitch=8, y_bstride=48, cb=0x20000, cr=0x30000, c_pitch=4, c_step=1, c_bstride=24, sub_x=1, sub_y=0, depth=8, msb=0)
    d.update(kw)
    return _lib.HatYuvSurface(**d)


BAD = {
    "odd w with sub_x = 1": (dict(), dict(w=7)),
    "odd h with sub_y = 1": (dict(sub_y=1, c_bstride=12), dict(h=5)),
    "cb null": (dict(cb=None), {}),
    "cr null": (dict(cr=None), {}),
    "y null": (dict(y=None), {}),
    "c_step 3": (dict(c_step=3), {}),
    "c_step 1 for words": (dict(depth=10, y_pitch=16, y_bstride=96, c_pitch=8, c_step=1, c_bstride=48), {}),
    "odd pitch for words": (dict(depth=10, y_pitch=17, y_bstride=120, c_pitch=8, c_step=2, c_bstride=48), {}),
    "odd chroma pitch for words": (dict(depth=10, y_pitch=16, y_bstride=96, c_pitch=9, c_step=2, c_bstride=64), {}),
    "odd pointer for words": (dict(depth=10, y=0x10001, y_pitch=16, y_bstride=96, c_pitch=8, c_step=2, c_bstride=48), {}),
    "overlapping luma batch stride": (dict(y_bstride=47), {}),
    "overlapping chroma batch stride": (dict(c_bstride=23), {}),
    "short luma pitch": (dict(y_pitch=7), {}),
    "short chroma pitch": (dict(c_step=2, c_pitch=7), {}),
    "4:4:0": (dict(sub_x=0, sub_y=1, c_pitch=8, c_bstride=24), {}),
    "sub_x 2": (dict(sub_x=2), {}),
    "depth 9": (dict(depth=9), {}),
    "msb 2": (dict(msb=2), {}),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_surfaces_are_refused_without_a_gpu(lib, name):
    kw, size = BAD[name]
    s = _surf(**kw)
    B, h, w = 2, size.get("h", 6), size.get("w", 8)
    m = (C.c_float * 12)(*yuv.csc()[0])
    fake = 0x40000
    assert lib.hat_yuv_to_planes(C.byref(s), fake, B, h, w, h, w, m, None) == EINVAL
    assert lib.hat_planes_to_yuv(fake, B, 16, 16, C.byref(s), h, w, m, None) == EINVAL
    mean = (C.c_float * 4)()
    assert lib.hat_conv3x3_to_yuv(fake, fake, fake, C.byref(s), B, 16, 16, 64, 64, h, w, 1.0, mean, m, 1, None) == EINVAL


def test_more_refusals_without_a_gpu(lib):
    m = (C.c_float * 12)(*yuv.csc()[0])
    fake, good = 0x40000, _surf()
    assert lib.hat_yuv_to_planes(None, fake, 2, 6, 8, 6, 8, m, None) == EINVAL
    assert lib.hat_yuv_to_planes(C.byref(good), None, 2, 6, 8, 6, 8, m, None) == EINVAL
    assert lib.hat_yuv_to_planes(C.byref(good), fake, 2, 6, 8, 12, 8, m, None) == EINVAL, "padding >= size"
    assert lib.hat_yuv_to_planes(C.byref(good), fake, 2, 6, 8, 6, 16, m, None) == EINVAL, "padding >= size"
    assert lib.hat_planes_to_yuv(fake, 2, 5, 16, C.byref(good), 6, 8, m, None) == EINVAL, "crop outside the planes"
    assert lib.hat_planes_to_yuv(None, 2, 16, 16, C.byref(good), 6, 8, m, None) == EINVAL
    assert lib.hat_plan_forward_yuv(None, C.byref(good), C.byref(good), 6, 8, m, m, None) == EINVAL
    mean = (C.c_float * 4)()
    assert lib.hat_conv3x3_to_yuv(fake, fake, fake, C.byref(good), 2, 16, 24, 64, 64, 6, 8, 1.0, mean, m, 1, None) == EINVAL, "W % 16"


def test_c_example_compiles_and_links(lib, tmp_path):
    exe = tmp_path / "plan_upscale_y4m_chroma"
    r = subprocess.run(["gcc", "-Wall", os.path.join(ROOT, "examples", "plan_upscale_y4m_chroma.c"), "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-2000:]
    assert exe.exists()


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_yuv420_views_are_yuv_views(fmt, dtype):
    """ops.yuv420_views is ops.yuv_views for the 4:2:0 layouts: the same pointers, shapes and strides (a batch stride larger than a
    frame and a storage offset included); it still refuses every other layout."""
    import torch
    from super_resolution_amd import ops
    B, h, w = 2, 6, 10
    rows = yuv.frame_shape(h, w)[0]
    f = torch.zeros(B, rows + 3, w, dtype=torch.uint8) if dtype == "uint8" else torch.zeros(B, rows + 3, w, dtype=torch.int16).view(torch.uint16)
    f = f[:, 1:1 + rows]
    a, b = ops.yuv420_views(f, fmt), ops.yuv_views(f, fmt)
    step = 1 if fmt == "i420" else 2
    for va, vb, shape in zip(a, b, ((B, h, w), (B, h // 2, w // 2), (B, h // 2, w // 2))):
        assert va.data_ptr() == vb.data_ptr() and tuple(va.shape) == tuple(vb.shape) == shape and va.stride() == vb.stride()
    assert a[1].stride(2) == a[2].stride(2) == step and a[1].data_ptr() != a[2].data_ptr()
    with pytest.raises(RuntimeError, match="format"):
        ops.yuv420_views(f, "i444")
