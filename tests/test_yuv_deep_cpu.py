"""10 / 12 / 16-bit 4:2:0 without a GPU: the numpy definition in super_resolution_amd/yuv.py (depth, containers, 'bt2020nc') is tied
to the 8-bit definition that tests/test_yuv_cpu.py pins to the reference; the four deep C entries refuse bad arguments before
they touch a device; Y4M with deep=True; the video command line; the C example is still plain C."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from super_resolution_amd import y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DEEP = (10, 12, 16)


# ---------------------------------------------------------------------------------------------- matrices
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020nc"])
def test_limited_range_matrices_do_not_depend_on_the_depth(matrix):
    to8, fr8 = yuv.csc(matrix, False, 8)
    for d in DEEP:
        to, fr = yuv.csc(matrix, False, d)
        assert to.dtype == np.float32 and fr.dtype == np.float32
        assert np.array_equal(to, to8) and np.array_equal(fr, fr8), d
    assert np.array_equal(yuv.csc(matrix, False)[0], to8), "depth defaults to 8"
    assert not np.array_equal(yuv.csc(matrix, True, 10)[1], yuv.csc(matrix, True, 8)[1]), "full range: 255.75 replaces 255"


def _one(code, depth, full, matrix="bt601"):
    f = yuv.join(*[np.full((1, 2 // s, 2 // s), c, dtype=np.uint16) for c, s in zip(code, (1, 2, 2))], "i420", depth)
    return yuv.yuv420_to_planes(f, fmt="i420", matrix=matrix, full_range=full, depth=depth)[0, :, 0, 0]


def test_known_answers_10_bit():
    """The bar of test_yuv_cpu.test_known_answers for black and white: 5e-6 (the constants' own rounding)."""
    for matrix in ("bt601", "bt709", "bt2020nc"):
        assert np.abs(_one((64, 512, 512), 10, False, matrix) - 0.0).max() <= 5e-6
        assert np.abs(_one((940, 512, 512), 10, False, matrix) - 1.0).max() <= 5e-6
        assert np.abs(_one((1023, 512, 512), 10, True, matrix) - 1.0).max() <= 5e-6
        assert np.abs(_one((0, 512, 512), 10, True, matrix) - 0.0).max() <= 5e-6
    # and the other way: the codes of black, white and mid-grey
    planes = np.repeat(np.repeat(np.array([0, 1, 0.5], dtype=np.float32)[None, None, None, :], 3, 1), 2, 2).repeat(2, 3)
    f = yuv.planes_to_yuv420(planes, fmt="i420", out_depth=10)
    assert f.dtype == np.uint16
    Y, Cb, Cr = yuv.split(f, "i420", 10)
    assert Y[0, 0, ::2].tolist() == [64, 940, 502] and Cb[0, 0].tolist() == [512] * 3 and Cr[0, 0].tolist() == [512] * 3
    f = yuv.planes_to_yuv420(planes, fmt="i420", full_range=True, out_depth=10)
    assert yuv.split(f, "i420")[0][0, 0, ::2].tolist() == [0, 1023, 512]     # 511.5 rounds half to even


def test_bt2020_primaries():
    """Y, Cb, Cr of red, green and blue against fp64 values derived from Kr / Kb here; within 1.5 code steps as the 8-bit codes
    of test_known_answers are (the codes are rounded: 0.5, plus the fp32 matrix)."""
    kr, kb = 0.2627, 0.0593
    kg = 1.0 - kr - kb
    rgb = np.eye(3)
    for depth, full in ((10, False), (10, True), (12, False), (16, True)):
        k = depth - 8
        if full:
            top = (2 ** depth - 1)
            ys = cs = top
            oy, oc = 0.0, 2.0 ** (depth - 1)
        else:
            ys, cs, oy, oc = 219.0 * 2 ** k, 224.0 * 2 ** k, 16.0 * 2 ** k, 128.0 * 2 ** k
        want = []
        for r, g, b in rgb:
            y = kr * r + kg * g + kb * b
            want.append((oy + ys * y, oc + cs * (b - y) / (2 * (1 - kb)), oc + cs * (r - y) / (2 * (1 - kr))))
        planes = np.repeat(np.repeat(rgb.T.astype(np.float32)[None, :, None, :], 2, 2), 2, 3)     # (1,3,2,6): one block per primary
        f = yuv.planes_to_yuv420(planes, fmt="i420", matrix="bt2020nc", full_range=full, out_depth=depth)
        Y, Cb, Cr = yuv.split(f, "i420", depth)
        for i in range(3):
            got = (int(Y[0, 0, 2 * i]), int(Cb[0, 0, i]), int(Cr[0, 0, i]))
            lim = [min(max(v, 0), 2 ** depth - 1) for v in want[i]]
            assert max(abs(a - b) for a, b in zip(got, lim)) <= 0.5 + 2.0 ** k * 1e-3, (depth, full, i, got, want[i])
        back = yuv.yuv420_to_planes(f, fmt="i420", matrix="bt2020nc", full_range=full, depth=depth)
        assert np.abs(back - planes).max() <= 3 * 1.5 / (219.0 * 2 ** k), (depth, full)
    with pytest.raises(RuntimeError, match="matrix"):
        yuv.csc("bt2020")                                          # the bare name stays refused: it is ambiguous


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_eight_bit_identity(fmt):
    """A deep frame that holds 8-bit codes times 2^k is the 8-bit frame, bit for bit, in limited range (the matrices are the
    same floats and s = code * 2^-k is exact); so is the MSB form f << 8 at any depth."""
    f = np.random.default_rng(5).integers(0, 256, (2, 18, 20), dtype=np.uint8)
    for matrix in ("bt601", "bt709"):
        ref = yuv.yuv420_to_planes(f, fmt=fmt, matrix=matrix, pad=(4, 6))
        for n in DEEP:
            deep = f.astype(np.uint16) << (n - 8)
            assert np.array_equal(yuv.yuv420_to_planes(deep, fmt=fmt, matrix=matrix, pad=(4, 6), depth=n, msb=False), ref), n
            assert np.array_equal(yuv.yuv420_to_planes(f.astype(np.uint16) << 8, fmt=fmt, matrix=matrix, pad=(4, 6), depth=n, msb=True), ref), n
    planes = np.random.default_rng(6).random((2, 3, 12, 20), dtype=np.float32) * 1.4 - 0.2
    assert np.array_equal(yuv.planes_to_yuv420(planes, fmt=fmt, out_depth=8), yuv.planes_to_yuv420(planes, fmt=fmt)), "k = 0 is the byte rule"


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("depth", DEEP)
def test_grey_ramp_survives(depth, full):
    """Every legal Y code with neutral chroma -> planes -> the same code.  The fp32 error of both matrices together is below
    0.03 code units at 16 bits (two roundings of ~65535 x 6e-8 x 3 terms), far from the 0.5 a wrong code needs."""
    k = depth - 8
    lo, hi = (0, 2 ** depth - 1) if full else (16 << k, 235 << k)
    codes = np.arange(lo, hi + 1, dtype=np.uint16)
    n = codes.size + (-codes.size) % 2
    Yrow = np.concatenate([codes, codes[-1:].repeat(n - codes.size)])
    Y = np.stack([Yrow, Yrow])[None]
    C_ = np.full((1, 1, n // 2), 1 << (depth - 1), dtype=np.uint16)
    for fmt, msb in (("i420", None), ("nv12", None), ("nv21", False)):
        f = yuv.join(yuv.encode(Y, depth, fmt, msb), yuv.encode(C_, depth, fmt, msb), yuv.encode(C_, depth, fmt, msb), fmt, depth, msb)
        planes = yuv.yuv420_to_planes(f, fmt=fmt, full_range=full, depth=depth, msb=msb)
        assert np.abs(planes[:, 0] - planes[:, 1]).max() <= 1e-5, "grey"
        back = yuv.planes_to_yuv420(planes, fmt=fmt, full_range=full, out_depth=depth, msb=msb)
        assert back.dtype == np.uint16 and np.array_equal(back, f), (fmt, msb)


def test_container_rules():
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 1024, (1, 6, 8), dtype=np.uint16)
    low = rng.integers(0, 64, (1, 6, 8), dtype=np.uint16)
    a = yuv.yuv420_to_planes(codes << 6, fmt="nv12", depth=10)                                   # nv12 defaults to MSB-aligned
    assert np.array_equal(yuv.yuv420_to_planes((codes << 6) | low, fmt="nv12", depth=10), a), "MSB: the low bits are ignored"
    assert np.array_equal(yuv.yuv420_to_planes(codes, fmt="nv12", depth=10, msb=False), a), "the keyword overrides the default"
    assert np.array_equal(yuv.yuv420_to_planes(codes.reshape(1, 6, 8), fmt="i420", depth=10),
                          yuv.yuv420_to_planes(codes << 6, fmt="i420", depth=10, msb=True)), "i420 defaults to LSB-aligned"
    over = codes.copy()
    over[0, 0, :4] = [1024, 4095, 40000, 65535]
    sat = codes.copy()
    sat[0, 0, :4] = 1023
    assert np.array_equal(yuv.yuv420_to_planes(over, fmt="i420", depth=10), yuv.yuv420_to_planes(sat, fmt="i420", depth=10)), "LSB words saturate"
    planes = rng.random((1, 3, 4, 8), dtype=np.float32)
    lsb = yuv.planes_to_yuv420(planes, fmt="nv12", out_depth=10, msb=False)
    msb = yuv.planes_to_yuv420(planes, fmt="nv12", out_depth=10)
    assert int(lsb.max()) <= 1023 and np.array_equal(msb, lsb << 6), "output words are code << shift"
    assert np.array_equal(yuv.planes_to_yuv420(planes, fmt="i420", out_depth=16, msb=True), yuv.planes_to_yuv420(planes, fmt="i420", out_depth=16, msb=False))
    assert np.array_equal(yuv.decode(msb, 10, "nv12"), lsb) and np.array_equal(yuv.encode(lsb, 10, "nv12"), msb)
    # the code is the byte-unit value times 2^k, rounded half to even: 0.5 grey is 125.5 -> 502, and 125.625 -> 502.5 -> 502
    y = yuv.planes_to_yuv420(np.full((1, 3, 2, 2), 0.5, dtype=np.float32), fmt="i420", out_depth=10)
    assert int(y[0, 0, 0]) == 502
    with pytest.raises(RuntimeError, match="uint16"):
        yuv.yuv420_to_planes(np.zeros((6, 8), dtype=np.uint8), depth=10)
    with pytest.raises(RuntimeError, match="uint8"):
        yuv.yuv420_to_planes(np.zeros((6, 8), dtype=np.uint16))
    with pytest.raises(RuntimeError, match="depth"):
        yuv.csc("bt601", False, 9)
    with pytest.raises(RuntimeError, match="depth"):
        yuv.planes_to_yuv420(planes, out_depth=14)
    with pytest.raises(RuntimeError, match="even"):
        yuv.yuv420_to_planes(np.zeros((15, 9), dtype=np.uint16), depth=10)


# ---------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    """Host memory standing in for device pointers: a call that is refused never dereferences them."""
    return C.create_string_buffer(4096)


def _m12():
    return (C.c_float * 12)(*yuv.csc()[0])


def _common_refusals(call):
    for d in (8, 9, 11, 14, 0, -10, 32):
        assert call(depth=d) == EINVAL, d
    assert call(msb=2) == EINVAL and call(msb=-1) == EINVAL
    assert call(y_pitch=41) == EINVAL and call(c_pitch=41) == EINVAL             # odd pitches
    assert call(c_step=1) == EINVAL and call(c_step=3) == EINVAL and call(c_step=8) == EINVAL and call(c_step=0) == EINVAL


def test_yuv420p16_to_planes_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem) // 16 * 16 + 16
    ok = dict(y=p, y_pitch=40, y_bstride=40 * 10, cb=p, cr=p, c_pitch=40, c_step=4, c_bstride=40 * 5, dst=p, B=1, h=10, w=20, Hp=16, Wp=32,
              m=_m12(), depth=10, msb=1)
    call = lambda **kw: lib.hat_yuv420p16_to_planes(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("y", "cb", "cr", "dst", "m"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("y", "cb", "cr"):
        assert call(**{k: p + 1}) == EINVAL, k                                   # a word is 2-byte aligned
    _common_refusals(call)
    assert call(B=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(h=9) == EINVAL and call(w=19) == EINVAL
    assert call(y_pitch=38) == EINVAL                                            # y_pitch < 2 w
    assert call(c_pitch=38) == EINVAL and call(c_step=2, c_pitch=18) == EINVAL   # c_pitch < c_step w / 2
    assert call(Hp=8) == EINVAL and call(Wp=18) == EINVAL and call(Hp=20) == EINVAL and call(Wp=40) == EINVAL
    assert call(B=2, y_bstride=40 * 9) == EINVAL and call(B=2, c_bstride=40 * 4) == EINVAL and call(B=2, y_bstride=40 * 10 + 1) == EINVAL


def test_planes_to_yuv420p16_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem) // 16 * 16 + 16
    ok = dict(src=p, B=1, Hs=16, Ws=32, y=p, y_pitch=60, y_bstride=60 * 12, cb=p, cr=p, c_pitch=30, c_step=2, c_bstride=30 * 6, h=12, w=30,
              m=_m12(), depth=12, msb=0)
    call = lambda **kw: lib.hat_planes_to_yuv420p16(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("src", "y", "cb", "cr", "m"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("y", "cb", "cr"):
        assert call(**{k: p + 1}) == EINVAL, k
    for d in (8, 9, 11, 14, 0, 32):
        assert call(depth=d) == EINVAL, d
    assert call(msb=2) == EINVAL
    assert call(y_pitch=61) == EINVAL and call(c_pitch=31) == EINVAL
    assert call(c_step=1) == EINVAL and call(c_step=3) == EINVAL and call(c_step=0) == EINVAL
    assert call(B=0) == EINVAL and call(Hs=0) == EINVAL and call(Ws=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(h=11) == EINVAL and call(w=29) == EINVAL
    assert call(y_pitch=58) == EINVAL and call(c_pitch=28) == EINVAL and call(c_step=4, c_pitch=58) == EINVAL
    assert call(h=18) == EINVAL and call(w=34, y_pitch=68, c_pitch=34) == EINVAL   # crop larger than the source
    assert call(B=2, y_bstride=60 * 11) == EINVAL and call(B=2, c_bstride=30 * 5) == EINVAL and call(B=2, c_bstride=30 * 6 + 1) == EINVAL


def test_conv3x3_to_yuv420p16_rejects_bad_arguments(lib, mem):
    from super_resolution_amd import _lib
    p = C.addressof(mem) // 16 * 16 + 16
    mean = (C.c_float * 4)(0.4488, 0.4371, 0.4040, 0.0)
    ok = dict(x=p, wpk=p, bias=p, y=p, y_pitch=60, y_bstride=60 * 12, cb=p, cr=p, c_pitch=60, c_step=4, c_bstride=60 * 6, B=1, H=16, W=32, Cc=64,
              ldx=64, h=12, w=30, scale=1.0, mean=mean, m=_m12(), dtype=_lib.HAT_BF16, depth=10, msb=1)
    call = lambda **kw: lib.hat_conv3x3_to_yuv420p16(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("x", "wpk", "bias", "y", "cb", "cr", "mean", "m"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("y", "cb", "cr"):
        assert call(**{k: p + 1}) == EINVAL, k
    for d in (8, 9, 11, 14, 0, 32):
        assert call(depth=d) == EINVAL, d
    assert call(msb=2) == EINVAL
    assert call(y_pitch=61) == EINVAL and call(c_pitch=61) == EINVAL
    assert call(c_step=1) == EINVAL and call(c_step=3) == EINVAL and call(c_step=0) == EINVAL
    assert call(B=0) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(W=40) == EINVAL                                              # the row sweep needs W % 16 == 0
    assert call(h=11) == EINVAL and call(w=29) == EINVAL
    assert call(y_pitch=58) == EINVAL and call(c_pitch=58) == EINVAL and call(c_step=2, c_pitch=28) == EINVAL
    assert call(h=18) == EINVAL and call(w=34, y_pitch=68, c_pitch=68) == EINVAL
    assert call(B=2, y_bstride=60 * 11) == EINVAL
    assert call(x=p + 2) == EINVAL                                           # fragment loads are 16-byte aligned
    assert call(dtype=_lib.HAT_F32) == -3 and call(Cc=48) == -3               # HAT_EUNSUPPORTED: only the bf16 conv_last shape is built


def test_plan_forward_yuv420_deep_rejects_bad_arguments(lib, mem):
    """What needs no plan is checked before the plan is read (a stand-in handle is never dereferenced); the checks against the
    plan's shape are tests/test_gpu_yuv_deep.py's."""
    p = C.addressof(mem) // 16 * 16 + 16
    ok = dict(plan=p, sy=p, sy_pitch=40, sy_bs=0, scb=p, scr=p, sc_pitch=20, sc_step=2, sc_bs=0, sd=10, sm=0, h=10, w=20,
              dy=p, dy_pitch=80, dy_bs=0, dcb=p, dcr=p, dc_pitch=40, dc_step=2, dc_bs=0, dd=10, dm=0, to=_m12(), fr=_m12())
    call = lambda **kw: lib.hat_plan_forward_yuv420_deep(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("plan", "sy", "scb", "scr", "dy", "dcb", "dcr", "to", "fr"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("sy", "scb", "scr", "dy", "dcb", "dcr"):
        assert call(**{k: p + 1}) == EINVAL, k
    assert call(h=0) == EINVAL and call(w=0) == EINVAL and call(h=9) == EINVAL and call(w=19) == EINVAL
    for d in (9, 11, 14, 0, 32, -8):
        assert call(sd=d) == EINVAL and call(dd=d) == EINVAL, d
    assert call(sm=2) == EINVAL and call(dm=2) == EINVAL and call(sm=-1) == EINVAL
    assert call(sc_step=1) == EINVAL and call(sc_step=3) == EINVAL and call(dc_step=1) == EINVAL and call(dc_step=3) == EINVAL
    assert call(sy_pitch=38) == EINVAL and call(sy_pitch=41) == EINVAL and call(sc_pitch=18) == EINVAL and call(sc_pitch=21) == EINVAL
    assert call(sc_step=4, sc_pitch=38) == EINVAL
    # a depth of 8 on a side means bytes there: the byte rules hold for that side
    assert call(sd=8, sc_step=4) == EINVAL and call(sd=8, sc_step=1, sy_pitch=19) == EINVAL and call(dd=8, dc_step=4) == EINVAL


# ---------------------------------------------------------------------------------------------- Y4M
def _frames(seed, n, h, w, top=1024):
    return [np.random.default_rng(seed + i).integers(0, top, (3 * h // 2, w), dtype=np.uint16) for i in range(n)]


def test_y4m_deep_writer_then_reader_is_the_identity(tmp_path):
    hdr = {"W": 22, "H": 14, "F": "30000:1001", "I": "p", "A": "1:1", "C": "420p10", "X": ["COLORRANGE=LIMITED"]}
    frames = _frames(1, 3, 14, 22)
    path = tmp_path / "a.y4m"
    with y4m.Writer(str(path), hdr, deep=True) as wr:
        for f in frames:
            wr.write(f)
        with pytest.raises(y4m.Y4MError, match="uint16"):
            wr.write(frames[0].astype(np.uint8))
    raw = path.read_bytes()
    assert raw.startswith(b"YUV4MPEG2 W22 H14 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\nFRAME\n")
    n0 = raw.index(b"\n") + 1
    assert len(raw) == n0 + 3 * (6 + 3 * 22 * 14), "a frame record is 3 w h bytes"
    assert raw[n0 + 6:n0 + 8] == int(frames[0][0, 0]).to_bytes(2, "little"), "little-endian words"
    with y4m.Reader(str(path), deep=True) as rd:
        assert rd.header == hdr and (rd.w, rd.h, rd.depth) == (22, 14, 10) and y4m.depth(rd.header) == 10
        got = list(rd)
    assert len(got) == 3 and all(g.dtype == np.uint16 and np.array_equal(a, b) for g, (a, b) in zip(got, zip(got, frames)))
    for c, d in (("420p10", 10), ("420p12", 12), ("420p16", 16), ("420", 8), ("420jpeg", 8)):
        h = y4m.parse_header(b"YUV4MPEG2 W4 H2 C" + c.encode(), deep=True)
        assert h["C"] == c and y4m.depth(h) == d
    assert y4m.depth(y4m.parse_header(b"YUV4MPEG2 W4 H2")) == 8
    # an 8-bit stream through the deep reader is what it was
    buf = io.BytesIO(b"YUV4MPEG2 W4 H2\nFRAME\n" + bytes(range(12)))
    (a,) = list(y4m.Reader(buf, deep=True))
    assert a.dtype == np.uint8 and a.reshape(-1).tolist() == list(range(12))


def test_y4m_default_still_refuses_deep_streams():
    with pytest.raises(y4m.Y4MError, match="C420p10.*8 bits"):
        y4m.parse_header(b"YUV4MPEG2 W4 H4 C420p10")
    with pytest.raises(y4m.Y4MError, match="colour space C420p10 has more than 8 bits per sample: only 8-bit 4:2:0 is supported"):
        y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H4 C420p10\n"))
    with pytest.raises(y4m.Y4MError, match="8 bits"):
        y4m.Writer(io.BytesIO(), {"W": 4, "H": 2, "C": "420p12"})
    with pytest.raises(y4m.Y4MError, match="C420p14"):
        y4m.parse_header(b"YUV4MPEG2 W4 H4 C420p14", deep=True)
    with pytest.raises(y4m.Y4MError, match="C444p10"):
        y4m.parse_header(b"YUV4MPEG2 W4 H4 C444p10", deep=True)
    with pytest.raises(y4m.Y4MError, match="truncated"):
        next(y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H2 C420p10\nFRAME\n" + bytes(12)), deep=True))


def test_scaled_header_keeps_the_colour_token():
    hdr = y4m.parse_header(b"YUV4MPEG2 W1280 H720 F25:1 C420p10 XFOO", deep=True)
    out = y4m.scaled_header(hdr, 4)
    assert out == {"W": 5120, "H": 2880, "F": "25:1", "C": "420p10", "X": ["FOO"]}
    assert y4m.format_header(out, deep=True) == b"YUV4MPEG2 W5120 H2880 F25:1 C420p10 XFOO\n"
    assert y4m.with_depth(out, 10) == out and y4m.with_depth(out, 8)["C"] == "420" and y4m.with_depth(out, 12)["C"] == "420p12"
    assert y4m.with_depth({"W": 4, "H": 2, "C": "420mpeg2", "X": []}, 8)["C"] == "420mpeg2", "an 8-bit token is kept"
    assert y4m.with_depth({"W": 4, "H": 2, "X": []}, 10)["C"] == "420p10"


def test_video_out_depth_and_command_line(tmp_path, monkeypatch):
    """upscale_file with the device part replaced by a stand-in that repeats every sample s times in both directions and converts
    the width by shifting; it records how it was called."""
    from super_resolution_amd import frames, video
    hdr = {"W": 6, "H": 4, "F": "24:1", "C": "420p10", "X": []}
    seq = _frames(9, 3, 4, 6)
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr, deep=True) as wr:
        for f in seq:
            wr.write(f)
    calls = []

    class Net:
        upscale = 2

    def fake(net, it, **kw):
        calls.append(kw)
        for a in it:
            a = np.repeat(np.repeat(a, 2, 0), 2, 1)
            yield a if kw["out_depth"] == kw["depth"] else (a >> 2).astype(np.uint8)

    monkeypatch.setattr(frames, "upscale_frames", fake)
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), matrix="bt2020nc")
    assert info == {"frames": 3, "in": (6, 4), "out": (12, 8), "depth": 10, "out_depth": 10}
    assert calls == [{"pixfmt": "i420", "matrix": "bt2020nc", "full_range": False, "depth": 10, "out_depth": 10}]
    with y4m.Reader(str(tmp_path / "out.y4m"), deep=True) as rd:
        assert rd.header == dict(hdr, W=12, H=8)
        got = list(rd)
    assert len(got) == 3 and all(np.array_equal(g, np.repeat(np.repeat(a, 2, 0), 2, 1)) for g, a in zip(got, seq))
    video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out8.y4m"), out_depth=8)
    assert calls[-1]["out_depth"] == 8 and calls[-1]["depth"] == 10
    with y4m.Reader(str(tmp_path / "out8.y4m")) as rd:            # the default reader: an 8-bit stream
        assert rd.header["C"] == "420"
        assert np.array_equal(next(rd), (np.repeat(np.repeat(seq[0], 2, 0), 2, 1) >> 2).astype(np.uint8))
    base = ["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m"]
    assert video.parser().parse_args(base).out_depth is None
    args = video.parser().parse_args(base + ["--out-depth", "10", "--matrix", "bt2020nc"])
    assert (args.out_depth, args.matrix) == (10, "bt2020nc")
    for bad in (["--out-depth", "9"], ["--out-depth", "ten"], ["--matrix", "bt2020"]):
        with pytest.raises(SystemExit):
            video.parser().parse_args(base + bad)


def test_y4m_example_is_still_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from super_resolution_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    exe = tmp_path / "plan_upscale_y4m"
    src = os.path.join(ROOT, "examples", "plan_upscale_y4m.c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", src, "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(src).read()
    assert "hat_plan_forward_yuv420_deep" in text and "C420p10" in text
