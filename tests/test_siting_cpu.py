"""Chroma siting on the host: the definition of super_resolution_amd/yuv.py ("Chroma siting": chroma_up, chroma_down and the siting=
arguments), the Y4M tokens, the video tool's arguments, and the C surface of the sited entries, which needs no GPU.  Every
comparison of two definitions is array_equal; the phase and edge tests compare against values written out by hand."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from super_resolution_amd import y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
F = np.float32


def _frame(seed, h, w, fmt, depth=8, msb=None):
    dt, _, maxcode, shift = yuv.container(depth, fmt, msb)
    rng = np.random.default_rng(seed)
    return (rng.integers(0, maxcode + 1, (2,) + yuv.frame_shape_fmt(h, w, fmt)).astype(np.uint16) << shift).astype(dt)


def _planes(seed, shape):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * 1.2 - 0.1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1: centre is today; what a layout ignores
def test_sitings_and_codes():
    assert yuv.SITINGS == ("center", "left", "topleft") and [yuv.SITINGS.index(s) for s in yuv.SITINGS] == [0, 1, 2]
    assert yuv.cosited((1, 1), "left") == (True, False) and yuv.cosited((1, 1), "topleft") == (True, True)
    assert yuv.cosited((1, 0), "topleft") == (True, False) and yuv.cosited((0, 0), "topleft") == (False, False)
    assert yuv.cosited(None, "left") == (False, False) and yuv.cosited((1, 1), "center") == (False, False)
    for call in (lambda: yuv.yuv_to_planes(np.zeros((6, 4), np.uint8), fmt="i420", siting="right"),
                 lambda: yuv.planes_to_yuv(np.zeros((1, 3, 4, 4), F), fmt="i420", siting=1),
                 lambda: yuv.chroma_up(np.zeros((2, 2), F), 4, 4, (1, 1), "centre")):
        with pytest.raises(RuntimeError, match="SITINGS"):
            call()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("fmt", yuv.ALL_FORMATS)
def test_center_is_todays_function_and_unsubsampled_axes_ignore_the_siting(fmt, depth):
    sub_x, sub_y, _ = yuv.LAYOUTS[fmt]
    frame = _frame(1, 12, 10, fmt, depth)
    planes = _planes(2, (2, 3, 13, 14))
    kin = dict(fmt=fmt, matrix="bt709", depth=depth)
    kout = dict(fmt=fmt, matrix="bt709", out_depth=depth)
    for pad, crop in (((0, 0), (12, 10)), ((5, 3), (8, 6))):
        a, b = yuv.yuv_to_planes(frame, pad=pad, **kin), yuv.planes_to_yuv(planes, crop=crop, **kout)
        assert np.array_equal(yuv.yuv_to_planes(frame, pad=pad, siting="center", **kin), a)
        assert np.array_equal(yuv.planes_to_yuv(planes, crop=crop, siting="center", **kout), b)
        if fmt in yuv.FORMATS:
            assert np.array_equal(yuv.yuv420_to_planes(frame, pad=pad, siting="center", **kin), yuv.yuv420_to_planes(frame, pad=pad, **kin))
            assert np.array_equal(yuv.planes_to_yuv420(planes, crop=crop, siting="center", **kout), yuv.planes_to_yuv420(planes, crop=crop, **kout))
            for s in ("left", "topleft"):
                assert np.array_equal(yuv.yuv420_to_planes(frame, pad=pad, siting=s, **kin), yuv.yuv_to_planes(frame, pad=pad, siting=s, **kin))
                assert np.array_equal(yuv.planes_to_yuv420(planes, crop=crop, siting=s, **kout), yuv.planes_to_yuv(planes, crop=crop, siting=s, **kout))
        left = (yuv.yuv_to_planes(frame, pad=pad, siting="left", **kin), yuv.planes_to_yuv(planes, crop=crop, siting="left", **kout))
        top = (yuv.yuv_to_planes(frame, pad=pad, siting="topleft", **kin), yuv.planes_to_yuv(planes, crop=crop, siting="topleft", **kout))
        if not sub_x:                # 4:4:4 and grey: every siting is centre
            assert np.array_equal(left[0], a) and np.array_equal(top[0], a) and np.array_equal(left[1], b) and np.array_equal(top[1], b)
        else:
            assert not np.array_equal(left[0], a) and not np.array_equal(left[1], b), "a co-sited axis is another filter"
            if not sub_y:            # 4:2:2: top-left is left
                assert np.array_equal(top[0], left[0]) and np.array_equal(top[1], left[1])
            else:
                assert not np.array_equal(top[0], left[0]) and not np.array_equal(top[1], left[1])
            # Y does not know about chroma
            assert np.array_equal(yuv.split_fmt(left[1], fmt)[0], yuv.split_fmt(b, fmt)[0])


# ---------------------------------------------------------------------------------------------- 2: phase
def test_phase_horizontal():
    """A chroma ramp C[j] = 4 j sampled AT luma column 2 j is the line c(x) = 2 x: 'left' reconstructs it exactly (up to the clamped
    last column), 'center' paints the staircase; and the line c[x] = 2 x goes down to 4 j exactly under 'left' (from j = 1: the
    first tap is replicated), to 4 j + 1 — half a luma pixel to the right — under 'center'."""
    h, w = 4, 16
    x, j = np.arange(w, dtype=F), np.arange(w // 2, dtype=F)
    for sub in ((1, 0), (1, 1)):
        Cs = np.broadcast_to(4 * j, (h >> sub[1], w // 2)).astype(F)
        up = yuv.chroma_up(Cs, h, w, sub, "left")
        assert up.dtype == F and up.shape == (h, w)
        assert np.array_equal(up[:, :w - 1], np.broadcast_to(2 * x[:w - 1], (h, w - 1)))
        assert np.array_equal(up[:, w - 1], up[:, w - 2]), "the last odd column clamps to its own sample"
        assert np.array_equal(yuv.chroma_up(Cs, h, w, sub, "center"), np.broadcast_to(4 * (np.arange(w) // 2), (h, w)).astype(F))
        line = np.broadcast_to(2 * x, (h, w)).astype(F)
        down = yuv.chroma_down(line, sub, "left")
        assert down.dtype == F and down.shape == (h >> sub[1], w // 2)
        assert np.array_equal(down[:, 1:], np.broadcast_to(4 * j[1:], (h >> sub[1], w // 2 - 1)))
        assert np.array_equal(down[:, 0], np.full(h >> sub[1], 0.5, F)), "(c[0] + c[1]) + 2 c[0] = 2, a quarter of it"
        assert np.array_equal(yuv.chroma_down(line, sub, "center"), np.broadcast_to(4 * j + 1, (h >> sub[1], w // 2)).astype(F))
        assert np.array_equal(yuv.chroma_down(line, sub, "left", 128.0), down + F(128.0))


def test_phase_vertical():
    """The same pair along y for 'topleft' on 4:2:0; under 'left' the vertical axis still behaves as centre."""
    h, w = 16, 4
    y, i = np.arange(h, dtype=F), np.arange(h // 2, dtype=F)
    Cs = np.broadcast_to((4 * i)[:, None], (h // 2, w // 2)).astype(F)
    up = yuv.chroma_up(Cs, h, w, (1, 1), "topleft")
    assert np.array_equal(up[:h - 1], np.broadcast_to((2 * y[:h - 1])[:, None], (h - 1, w)))
    assert np.array_equal(up[h - 1], up[h - 2])
    stair = np.broadcast_to((4 * (np.arange(h) // 2))[:, None], (h, w)).astype(F)
    assert np.array_equal(yuv.chroma_up(Cs, h, w, (1, 1), "left"), stair) and np.array_equal(yuv.chroma_up(Cs, h, w, (1, 1), "center"), stair)
    line = np.broadcast_to((2 * y)[:, None], (h, w)).astype(F)
    down = yuv.chroma_down(line, (1, 1), "topleft")
    assert np.array_equal(down[1:], np.broadcast_to((4 * i[1:])[:, None], (h // 2 - 1, w // 2)))
    assert np.array_equal(down[0], np.full(w // 2, 0.5, F))
    box = np.broadcast_to((4 * i + 1)[:, None], (h // 2, w // 2)).astype(F)
    assert np.array_equal(yuv.chroma_down(line, (1, 1), "left"), box) and np.array_equal(yuv.chroma_down(line, (1, 1), "center"), box)


# ---------------------------------------------------------------------------------------------- 3: flat fields
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("fmt", ["nv12", "i420", "i422", "nv16"])
def test_flat_fields_do_not_see_the_siting(fmt, depth):
    """Planes constant per channel: every tap sums the same value, 4 c * 0.25, 8 c * 0.125 and 16 c * 0.0625 are c exactly, so all
    sitings write the same frame; and a frame with constant chroma goes in the same way under all of them."""
    planes = np.empty((2, 3, 8, 12), F)
    planes[:] = np.array([0.8125, 0.3, 0.517], F)[None, :, None, None]
    frames = [yuv.planes_to_yuv(planes, fmt=fmt, matrix="bt709", out_depth=depth, crop=(6, 10), siting=s) for s in yuv.SITINGS]
    assert np.array_equal(frames[1], frames[0]) and np.array_equal(frames[2], frames[0])
    src = _frame(3, 6, 10, fmt, depth)
    _, cb, cr = yuv.split_fmt(src, fmt)
    cb[...], cr[...] = yuv.encode(np.uint16(77 << (depth - 8)), depth, fmt), yuv.encode(np.uint16(201 << (depth - 8)), depth, fmt)
    ins = [yuv.yuv_to_planes(src, fmt=fmt, depth=depth, pad=(3, 5), siting=s) for s in yuv.SITINGS]
    assert np.array_equal(ins[1], ins[0]) and np.array_equal(ins[2], ins[0])


# ---------------------------------------------------------------------------------------------- 4: edges, by hand
def _chroma_in(frame, fmt, siting, pad=(0, 0)):
    """The Cb' + 128 that yuv_to_planes used, read back through a matrix whose R row is Cb' / 256 + 0.5 (exact for these values)."""
    to = np.zeros(12, F)
    to[1], to[3] = F(1 / 256), F(0.5)
    real = yuv.csc

    def fake(matrix="bt601", full_range=False, depth=8):
        return to, real(matrix, full_range, depth)[1]
    yuv.csc = fake
    try:
        r = yuv.yuv_to_planes(frame, fmt=fmt, pad=pad, siting=siting)[0, 0]
    finally:
        yuv.csc = real
    return (r - F(0.5)) * F(256) + F(128)


def test_edges_2x2_every_tap_clamped():
    # in: one chroma sample; every clamp lands on it
    frame = yuv.join_fmt(np.array([[10, 20], [30, 40]], np.uint8), np.array([[100]], np.uint8), np.array([[200]], np.uint8), "i420")
    for s in yuv.SITINGS:
        assert np.array_equal(_chroma_in(frame, "i420", s), np.full((2, 2), 100, F))
        assert np.array_equal(yuv.yuv_to_planes(frame, fmt="i420", siting=s), yuv.yuv_to_planes(frame, fmt="i420"))
    # out: c = [[a, b], [c, d]].  left: t_r = (c[r][0] + c[r][1]) + 2 c[r][0]; (t_0 + t_1) / 8.  topleft: ((t_0 + t_1) + 2 t_0) / 16.
    c = np.array([[8, 16], [32, 64]], F)
    assert np.array_equal(yuv.chroma_down(c, (1, 1), "center"), np.array([[30]], F))               # 120 / 4
    assert np.array_equal(yuv.chroma_down(c, (1, 1), "left"), np.array([[25]], F))                 # t = 40, 160: 200 / 8
    assert np.array_equal(yuv.chroma_down(c, (1, 1), "topleft"), np.array([[17.5]], F))            # (40 + 160) + 80 = 280 / 16
    assert np.array_equal(yuv.chroma_down(c, (1, 0), "left"), np.array([[10], [40]], F))           # 40 / 4, 160 / 4
    assert np.array_equal(yuv.chroma_down(c, (1, 0), "topleft"), np.array([[10], [40]], F))
    out = yuv.planes_to_yuv(_planes(5, (1, 3, 2, 2)), fmt="nv12", siting="topleft")
    assert out.shape == (1, 3, 2)


def test_edges_reflected_last_odd_column_interpolates_with_the_clamped_neighbour():
    """A 4 x 6 4:2:0 frame padded by (2, 3): chroma columns [10, 20, 40], rows [r0, r0 + 100].  Source columns 0 .. 5 under 'left'
    are 10, 15, 20, 30, 40, 40 (the last odd column has no right neighbour: it clamps), and the padded columns 6, 7, 8 read source
    columns 4, 3, 2 — the reflection comes first, the interpolation second."""
    Cb = np.array([[10, 20, 40], [110, 120, 140]], np.uint8)
    frame = yuv.join_fmt(np.zeros((4, 6), np.uint8), Cb, Cb, "i420")
    row0 = np.array([10, 15, 20, 30, 40, 40, 40, 30, 20], F)
    left = _chroma_in(frame, "i420", "left", pad=(2, 3))
    assert np.array_equal(left, np.stack([row0, row0, row0 + 100, row0 + 100, row0 + 100, row0]))   # rows 0 1 2 3 | 2 1
    top = _chroma_in(frame, "i420", "topleft", pad=(2, 3))
    assert np.array_equal(top, np.stack([row0, row0 + 50, row0 + 100, row0 + 100, row0 + 100, row0 + 50]))   # row 3 clamps; 4, 5 read 2, 1
    centre = np.array([10, 10, 20, 20, 40, 40, 40, 20, 20], F)
    assert np.array_equal(_chroma_in(frame, "i420", "center", pad=(2, 3)), np.stack([centre, centre, centre + 100, centre + 100, centre + 100, centre]))
    # 4:2:2, 10-bit codes: halves of a code are exact (s = code / 4)
    frame = yuv.join_fmt(np.zeros((1, 4), np.uint16), np.array([[401, 404]], np.uint16), np.array([[0, 0]], np.uint16), "i422", 10)
    to = np.zeros(12, F)
    to[1], to[3] = F(1 / 256), F(0.5)
    real = yuv.csc
    yuv.csc = lambda *a, **k: (to, None)
    try:
        r = yuv.yuv_to_planes(frame, fmt="i422", depth=10, pad=(0, 2), siting="left")[0, 0, 0]
    finally:
        yuv.csc = real
    assert np.array_equal((r - F(0.5)) * F(256) + F(128), np.array([100.25, 100.625, 101, 101, 101, 100.625], F))


def test_down_taps_by_hand():
    """One row of a 4:2:2 'left' down-sample and a 4 x 4 'topleft' one against the taps written out."""
    c = np.array([[1, 2, 4, 8, 16, 32]], F)
    assert np.array_equal(yuv.chroma_down(c, (1, 0), "left"), np.array([[(1 + 2 + 2) / 4, (2 + 8 + 8) / 4, (8 + 32 + 32) / 4]], F))
    c = np.arange(16, dtype=F).reshape(4, 4) ** 2
    t = np.stack([[(r[0] + r[1]) + 2 * r[0], (r[1] + r[3]) + 2 * r[2]] for r in c]).astype(F)
    want = np.stack([(t[0] + t[1]) + 2 * t[0], (t[1] + t[3]) + 2 * t[2]]) * F(0.0625)
    assert np.array_equal(yuv.chroma_down(c, (1, 1), "topleft"), want)
    assert np.array_equal(yuv.chroma_down(c, (1, 1), "left"), np.stack([t[0] + t[1], t[2] + t[3]]) * F(0.125))
    # a crop narrower than the planes: no tap reads past it
    planes = _planes(7, (1, 3, 6, 8))
    wide = planes.copy()
    wide[:, :, 4:, :], wide[:, :, :, 6:] = 0.25, 0.75
    for s in ("left", "topleft"):
        assert np.array_equal(yuv.planes_to_yuv(planes, fmt="i420", crop=(4, 6), siting=s), yuv.planes_to_yuv(wide, fmt="i420", crop=(4, 6), siting=s))


# ---------------------------------------------------------------------------------------------- 5: the C surface
@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


NAMES = ("hat_yuv_to_planes_sited", "hat_planes_to_yuv_sited", "hat_plan_forward_yuv_sited")


def test_symbols_are_declared_exported_and_bound(lib, tmp_path):
    from super_resolution_amd import _lib
    text = open(os.path.join(ROOT, "include", "hat_mi355x.h")).read()
    for name in NAMES:
        assert f"int {name}(" in text and name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.hat_abi_version() == 2 and "#define HAT_ABI_VERSION 2" in text.replace("  ", " ")
    # the surface keeps its size and the header its codes: a C program against the header
    prog = ('#include <stdio.h>\n#include "hat_mi355x.h"\nint main(){printf("%zu %d %d %d %d", sizeof(HatYuvSurface), HAT_SITING_CENTER, '
            'HAT_SITING_LEFT, HAT_SITING_TOPLEFT, HAT_ABI_VERSION);return 0;}\n')
    (tmp_path / "s.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [C.sizeof(_lib.HatYuvSurface), 0, 1, 2, 2] and C.sizeof(_lib.HatYuvSurface) == 80
    assert [f[0] for f in _lib.HatYuvSurface._fields_] == ["y", "y_pitch", "y_bstride", "cb", "cr", "c_pitch", "c_step", "c_bstride", "sub_x",
                                                          "sub_y", "depth", "msb"], "no siting field: it travels beside the surface"


def _surf(**kw):
    """A good 8-bit 4:2:0 planar surface of a (2, 6, 8) block at made-up (never dereferenced) addresses, then the changes."""
    from super_resolution_amd import _lib
    d = dict(y=0x10000, y_pitch=8, y_bstride=48, cb=0x20000, cr=0x30000, c_pitch=4, c_step=1, c_bstride=12, sub_x=1, sub_y=1, depth=8, msb=0)
    d.update(kw)
    return _lib.HatYuvSurface(**d)


def test_sited_entries_refuse_without_a_device(lib):
    m = (C.c_float * 12)(*yuv.csc()[0])
    fake, good = 0x40000, _surf()
    for siting in (-1, 3, 7):        # before anything else is looked at, and with everything else in order
        assert lib.hat_yuv_to_planes_sited(C.byref(good), siting, fake, 2, 6, 8, 6, 8, m, None) == EINVAL
        assert lib.hat_planes_to_yuv_sited(fake, 2, 16, 16, C.byref(good), siting, 6, 8, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(fake, C.byref(good), siting, C.byref(good), 0, 6, 8, m, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(fake, C.byref(good), 0, C.byref(good), siting, 6, 8, m, m, None) == EINVAL
    for siting in (0, 1, 2):         # NULL arguments and everything the unsited entries refuse
        assert lib.hat_yuv_to_planes_sited(None, siting, fake, 2, 6, 8, 6, 8, m, None) == EINVAL
        assert lib.hat_yuv_to_planes_sited(C.byref(good), siting, None, 2, 6, 8, 6, 8, m, None) == EINVAL
        assert lib.hat_yuv_to_planes_sited(C.byref(good), siting, fake, 2, 6, 8, 6, 8, None, None) == EINVAL
        assert lib.hat_yuv_to_planes_sited(C.byref(good), siting, fake, 2, 6, 8, 12, 8, m, None) == EINVAL, "padding >= size"
        assert lib.hat_yuv_to_planes_sited(C.byref(good), siting, fake, 2, 6, 7, 6, 7, m, None) == EINVAL, "odd w with sub_x = 1"
        assert lib.hat_planes_to_yuv_sited(None, 2, 16, 16, C.byref(good), siting, 6, 8, m, None) == EINVAL
        assert lib.hat_planes_to_yuv_sited(fake, 2, 16, 16, None, siting, 6, 8, m, None) == EINVAL
        assert lib.hat_planes_to_yuv_sited(fake, 2, 16, 16, C.byref(good), siting, 6, 8, None, None) == EINVAL
        assert lib.hat_planes_to_yuv_sited(fake, 2, 5, 16, C.byref(good), siting, 6, 8, m, None) == EINVAL, "crop outside the planes"
        assert lib.hat_planes_to_yuv_sited(fake, 2, 16, 16, C.byref(_surf(cr=None)), siting, 6, 8, m, None) == EINVAL
        assert lib.hat_planes_to_yuv_sited(fake, 2, 16, 16, C.byref(_surf(c_bstride=11)), siting, 6, 8, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(None, C.byref(good), siting, C.byref(good), siting, 6, 8, m, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(fake, None, siting, C.byref(good), siting, 6, 8, m, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(fake, C.byref(good), siting, None, siting, 6, 8, m, m, None) == EINVAL
        assert lib.hat_plan_forward_yuv_sited(fake, C.byref(good), siting, C.byref(good), siting, 6, 8, None, m, None) == EINVAL


def test_python_refuses_unknown_sitings_by_name():
    import torch
    from super_resolution_amd import ops
    with pytest.raises(RuntimeError, match="SITINGS"):
        ops._siting((1, 1), "bottom")
    assert ops._siting((1, 0), "topleft") == ("left", 1) and ops._siting(None, "left") == ("center", 0) and ops._siting((0, 0), "topleft")[1] == 0
    assert ops._siting((1, 1), "topleft") == ("topleft", 2)
    from super_resolution_amd import frames

    class Net(torch.nn.Module):
        upscale = 2
    with pytest.raises(RuntimeError, match="SITINGS"):
        next(frames.upscale_frames(Net(), iter([]), pixfmt="i420", siting="mpeg2"))
    with pytest.raises(RuntimeError, match="YCbCr"):
        next(frames.upscale_frames(Net(), iter([]), siting="left"))


def test_c_example_with_chroma_loc_compiles_and_refuses_bad_values(lib, tmp_path):
    exe = tmp_path / "plan_upscale_y4m_chroma"
    r = subprocess.run(["gcc", "-Wall", os.path.join(ROOT, "examples", "plan_upscale_y4m_chroma.c"), "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-2000:]
    text = open(os.path.join(ROOT, "examples", "plan_upscale_y4m_chroma.c")).read()
    assert "hat_plan_forward_yuv_sited(" in text and "--chroma-loc" in text


# ---------------------------------------------------------------------------------------------- 6: files and the tool
def test_siting_of_the_tokens():
    p = lambda s: y4m.parse_header(b"YUV4MPEG2 W4 H4 " + s, chroma=True)
    assert y4m.siting_of(p(b"C420mpeg2")) == "left" and y4m.siting_of(p(b"C420paldv")) == "topleft"
    assert y4m.siting_of(p(b"C420jpeg")) == "center" and y4m.siting_of(p(b"C420")) == "center" and y4m.siting_of(p(b"")) == "center"
    for c in (b"C420p10", b"C422", b"C422p10", b"C444", b"Cmono", b"Cmono12"):
        assert y4m.siting_of(p(c)) == "center", c
    assert y4m.siting_of(p(b"C420 XYSCSS=420MPEG2")) == "left" and y4m.siting_of(p(b"C420p10 XYSCSS=420PALDV")) == "topleft"
    assert y4m.siting_of(p(b"C420jpeg XYSCSS=420MPEG2")) == "left" and y4m.siting_of(p(b"C420p10 XYSCSS=420JPEG")) == "center"
    assert y4m.siting_of(p(b"XYSCSS=420MPEG2")) == "left" and y4m.siting_of(p(b"C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED")) == "center"
    assert y4m.siting_of(p(b"C420mpeg2 XYSCSS=420JPEG")) == "left", "a C token that names a siting other than centre decides"
    assert y4m.siting_of(p(b"C422 XYSCSS=422")) == "center", "a 4:2:2 header cannot say: the user asks for left"


def test_with_siting_rewrites_the_token_and_an_existing_xyscss():
    p = lambda s: y4m.parse_header(b"YUV4MPEG2 W4 H4 F25:1 " + s, chroma=True)
    for src in (b"C420jpeg", b"C420mpeg2", b"C420paldv"):
        for s, tok in (("center", "420jpeg"), ("left", "420mpeg2"), ("topleft", "420paldv")):
            out = y4m.with_siting(p(src), s)
            assert out["C"] == tok and y4m.siting_of(out) == s and out["F"] == "25:1"
    assert y4m.with_siting(p(b"C420"), "center")["C"] == "420" and y4m.with_siting(p(b"C420"), "left")["C"] == "420mpeg2"
    assert "C" not in y4m.with_siting(p(b""), "center") and y4m.with_siting(p(b""), "topleft")["C"] == "420paldv"
    deep = p(b"C420p10 XYSCSS=420JPEG XCOLORRANGE=LIMITED")
    out = y4m.with_siting(deep, "left")
    assert out["C"] == "420p10" and out["X"] == ["YSCSS=420MPEG2", "COLORRANGE=LIMITED"] and y4m.siting_of(out) == "left"
    assert deep["X"] == ["YSCSS=420JPEG", "COLORRANGE=LIMITED"], "the argument is not changed"
    both = y4m.with_siting(p(b"C420mpeg2 XYSCSS=420MPEG2"), "topleft")
    assert both["C"] == "420paldv" and both["X"] == ["YSCSS=420PALDV"]
    for c in (b"C422", b"C444p10", b"Cmono", b"C420p12"):
        assert y4m.with_siting(p(c), "left") == p(c), "nothing to rewrite: the token carries no siting"
    with pytest.raises(y4m.Y4MError, match="siting"):
        y4m.with_siting(p(b"C420"), "right")
    y4m.format_header(y4m.with_siting(p(b"C420"), "left"))       # (still a header the plain writer takes)


def test_video_parser_and_the_default_chroma_loc():
    from super_resolution_amd import video
    base = ["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m"]
    a = video.parser().parse_args(base)
    assert a.chroma_loc == "center" and a.out_chroma_loc is None
    for v in ("auto", "center", "left", "topleft"):
        a = video.parser().parse_args(base + ["--chroma-loc", v, "--out-chroma-loc", v])
        assert a.chroma_loc == v and a.out_chroma_loc == v
    for flag in ("--chroma-loc", "--out-chroma-loc"):
        with pytest.raises(SystemExit):
            video.parser().parse_args(base + [flag, "right"])
    mpeg2 = y4m.parse_header(b"YUV4MPEG2 W4 H4 C420mpeg2")
    assert video.resolve_chroma_loc(mpeg2) == ("center", "center"), "the default treats every stream as before"
    assert video.resolve_chroma_loc(mpeg2, "auto") == ("left", "left") and video.resolve_chroma_loc(mpeg2, "auto", "center") == ("left", "center")
    assert video.resolve_chroma_loc(mpeg2, "topleft", None) == ("topleft", "topleft") and video.resolve_chroma_loc(mpeg2, "center", "auto") == ("center", "left")
    with pytest.raises(RuntimeError, match="chroma location"):
        video.resolve_chroma_loc(mpeg2, "right")


def test_default_chroma_loc_leaves_a_mpeg2_header_and_its_treatment_as_today(tmp_path, monkeypatch):
    """upscale_file with the default on a C420mpeg2 file: the frames go to upscale_frames WITHOUT siting arguments (today's call,
    keyword for keyword), the header is copied with its token, and the info dict has no new keys; with 'auto' the same file is
    'left' on both sides and says so."""
    from super_resolution_amd import frames, video
    hdr = {"W": 4, "H": 4, "F": "25:1", "C": "420mpeg2", "X": []}
    src = [np.full((6, 4), 7 + i, np.uint8) for i in range(2)]
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr) as wr:
        for f in src:
            wr.write(f)
    calls = []

    def fake(net, rd, **kw):
        calls.append(kw)
        for f in rd:
            yield np.zeros((12, 8), np.uint8) + f[0, 0]

    monkeypatch.setattr(frames, "upscale_frames", fake)

    class Net:
        upscale = 2
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"))
    assert calls[-1] == dict(pixfmt="i420", matrix="bt601", full_range=False) and info == {"frames": 2, "in": (4, 4), "out": (8, 8)}
    with y4m.Reader(str(tmp_path / "out.y4m")) as rd:
        assert rd.header == y4m.scaled_header(hdr, 2) and len(list(rd)) == 2
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "auto.y4m"), chroma_loc="auto")
    assert calls[-1] == dict(pixfmt="i420", matrix="bt601", full_range=False, siting="left", out_siting="left")
    assert info["chroma_loc"] == "left" and info["out_chroma_loc"] == "left"
    with y4m.Reader(str(tmp_path / "auto.y4m")) as rd:
        assert rd.header["C"] == "420mpeg2"
    video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "tl.y4m"), chroma_loc="auto", out_chroma_loc="topleft")
    assert calls[-1]["siting"] == "left" and calls[-1]["out_siting"] == "topleft"
    with y4m.Reader(str(tmp_path / "tl.y4m")) as rd:
        assert rd.header["C"] == "420paldv", "the written header agrees with what was written"
    video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "c.y4m"), chroma_loc="left", out_chroma_loc="center")
    with y4m.Reader(str(tmp_path / "c.y4m")) as rd:
        assert rd.header["C"] == "420jpeg"
