"""Packed 4:2:2 (UYVY / YUY2 / Y210 / v210) without a GPU: the definition in super_resolution_amd/yuv.py (layouts against hand-written
rows, the composition through 'i422'), the C entries' refusals from the loaded library, the ctypes mirror of HatPackedSurface, the
C example, the headerless file reader / writer and the file tool's argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from super_resolution_amd import rawvideo, video, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uyvy", 8, None), ("yuy2", 8, None), ("y210", 10, None), ("y210", 10, False), ("y210", 12, None), ("y210", 16, None), ("v210", 10, None)]
IDS = ["uyvy", "yuy2", "y210", "y210lsb", "y212", "y216", "v210"]
EINVAL = -1


def _samples(seed, h, w, fmt, depth, msb, lead=()):
    """Random stored samples Y, Cb, Cr of an h x w frame: bytes, y210 words in their alignment (LSB words also above the code range:
    they saturate; MSB words carry low bits), v210 codes."""
    rng = np.random.default_rng(seed)
    if fmt in ("uyvy", "yuy2"):
        top, dt = 256, np.uint8
    elif fmt == "v210":
        top, dt = 1024, np.uint16
    else:
        top, dt = 65536, np.uint16
    return tuple(rng.integers(0, top, lead + (h, n)).astype(dt) for n in (w, w // 2, w // 2))


@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def test_format_tables_are_unchanged():
    assert yuv.FORMATS == ("nv12", "nv21", "i420")
    assert yuv.ALL_FORMATS == ("nv12", "nv21", "i420", "i422", "nv16", "i444", "nv24", "gray") == tuple(yuv.LAYOUTS)
    assert yuv.PACKED_FORMATS == ("uyvy", "yuy2", "y210", "v210")
    assert not set(yuv.PACKED_FORMATS) & set(yuv.LAYOUTS)


@pytest.mark.parametrize("fmt,depth,msb", CASES, ids=IDS)
@pytest.mark.parametrize("w", [2, 6, 8, 46, 48, 50])
def test_pack_unpack_round_trip(fmt, depth, msb, w):
    Y, Cb, Cr = _samples(w, 3, w, fmt, depth, msb, lead=(2,))
    frame = yuv.pack422(Y, Cb, Cr, fmt, depth, msb)
    assert frame.shape == (2,) + yuv.packed_shape(3, w, fmt) and frame.dtype == yuv.packed_container(fmt, depth, msb)[0]
    assert yuv.packed_size(frame.shape, fmt, width=w) == (3, w)
    for got, want in zip(yuv.unpack422(frame, fmt, w, depth, msb), (Y, Cb, Cr)):
        assert np.array_equal(got, want)
    assert np.array_equal(yuv.pack422(*yuv.unpack422(frame, fmt, w, depth, msb), fmt, depth, msb), frame)


def test_byte_and_word_order_against_hand_written_rows():
    Y, Cb, Cr = np.array([[10, 11, 12, 13]], np.uint8), np.array([[20, 21]], np.uint8), np.array([[30, 31]], np.uint8)
    assert yuv.pack422(Y, Cb, Cr, "uyvy").tolist() == [[20, 10, 30, 11, 21, 12, 31, 13]]
    assert yuv.pack422(Y, Cb, Cr, "yuy2").tolist() == [[10, 20, 11, 30, 12, 21, 13, 31]]
    w = lambda a: np.array(a, np.uint16)
    f = yuv.pack422(w([[0x0040, 0x0080]]), w([[0x00C0]]), w([[0x0100]]), "y210", 10)
    assert f.dtype == np.uint16 and f.tolist() == [[0x0040, 0x00C0, 0x0080, 0x0100]]
    assert f.astype("<u2").tobytes() == bytes([0x40, 0x00, 0xC0, 0x00, 0x80, 0x00, 0x00, 0x01])      # little-endian words
    # MSB-aligned by default: the stored word 0x0040 is the 10-bit code 1; msb=False reads the word as the code
    msb = yuv.packed_to_planes(f, fmt="y210", depth=10)
    lsb = yuv.packed_to_planes((f >> 6).astype(np.uint16), fmt="y210", depth=10, msb=False)
    assert np.array_equal(msb, lsb)
    assert yuv.packed_container("y210", None, None) == (np.uint16, 10, True) and yuv.packed_container("y210", 16, False)[2] is False


def test_v210_group_against_literal_words():
    Y = np.array([[0x001, 0x002, 0x003, 0x004, 0x005, 0x3FF]], np.uint16)
    Cb, Cr = np.array([[0x010, 0x020, 0x030]], np.uint16), np.array([[0x100, 0x200, 0x300]], np.uint16)
    f = yuv.pack422(Y, Cb, Cr, "v210")
    assert f.shape == (1, 128) and f.dtype == np.uint8
    # word 0: Cb0 Y0 Cr0; word 1: Y1 Cb1 Y2; word 2: Cr1 Y3 Cb2; word 3: Y4 Cr2 Y5 — codes at bits 0, 10, 20
    assert [hex(v) for v in f[0, :16].view("<u4")] == ["0x10000410", "0x308002", "0x3001200", "0x3ffc0005"]
    assert not f[0, 16:].any()
    for got, want in zip(yuv.unpack422(f, "v210", 6), (Y, Cb, Cr)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("w,row", [(2, 128), (46, 128), (48, 128), (50, 256), (96, 256), (98, 384)])
def test_v210_row_length_and_zeroed_tail(w, row):
    assert yuv.packed_shape(3, w, "v210") == (3, row)
    Y, Cb, Cr = (np.full(s, 1023, np.uint16) for s in ((3, w), (3, w // 2), (3, w // 2)))
    f = yuv.pack422(Y, Cb, Cr, "v210")
    words = f.view("<u4").reshape(3, row // 4)
    assert not (words >> 30).any()                                   # bits 30-31 of every word
    groups = -(-w // 6)
    assert not f[:, 16 * groups:].any()                              # every byte from the last group to the end of the row
    comp = np.stack([(words[:, :4 * groups] >> s) & 1023 for s in (0, 10, 20)], axis=-1).reshape(3, groups, 12)
    assert int((comp == 1023).sum()) == 3 * 2 * w and int((comp != 0).sum()) == 3 * 2 * w   # the codes past w are zero
    with pytest.raises(ValueError):
        yuv.packed_size(f.shape, "v210")                             # the shape does not give the width
    with pytest.raises(ValueError):
        yuv.packed_size((3, 2 * w), "uyvy", width=w + 2)              # optional and checked elsewhere


def test_v210_garbage_in_padding_and_top_bits_decodes_the_same():
    w = 50
    f = yuv.pack422(*_samples(5, 3, w, "v210", 10, None), "v210")
    g = f.copy()
    words = g.view("<u4").reshape(3, -1)
    words |= np.uint32(0xC0000000)                                    # bits 30-31
    groups = -(-w // 6)
    g[:, 16 * groups:] = 0xA5                                         # the row tail
    last = words[:, 4 * (groups - 1):4 * groups]                     # w % 6 = 2: pixels 2..5 of the last group are past w
    last[:, 1] |= np.uint32(0x3FF << 10) | np.uint32(0x3FF << 20)          # (bits 0-9 of word 1 are Y1, pixel 49)
    last[:, 2] |= np.uint32(0x3FFFFFFF)
    last[:, 3] |= np.uint32(0x3FFFFFFF)
    assert not np.array_equal(f, g)
    for kw in (dict(siting="center"), dict(siting="left", pad=(2, 49))):
        assert np.array_equal(yuv.packed_to_planes(f, fmt="v210", width=w, **kw), yuv.packed_to_planes(g, fmt="v210", width=w, **kw))


@pytest.mark.parametrize("fmt,depth,msb", CASES, ids=IDS)
@pytest.mark.parametrize("siting", ["center", "left"])
def test_definitions_are_the_i422_ones(fmt, depth, msb, siting):
    """packed_to_planes / planes_to_packed equal the composition through 'i422' written out here, and 'topleft' is 'left'."""
    h, w, B = 3, 50, 2
    emsb = yuv.packed_container(fmt, depth, msb)[2]
    Y, Cb, Cr = _samples(11, h, w, fmt, depth, msb, lead=(B,))
    frame = yuv.pack422(Y, Cb, Cr, fmt, depth, msb)
    kw = dict(matrix="bt709", full_range=True)
    want = yuv.yuv_to_planes(yuv.join_fmt(Y, Cb, Cr, "i422", depth, emsb), fmt="i422", depth=depth, msb=emsb, pad=(2, 49), siting=siting, **kw)
    got = yuv.packed_to_planes(frame, fmt=fmt, width=w, depth=depth, msb=msb, pad=(2, 49), siting=siting, **kw)
    assert got.shape == (B, 3, h + 2, w + 49) and np.array_equal(got, want)
    planes = np.random.default_rng(3).uniform(-0.2, 1.2, (B, 3, h + 1, w + 3)).astype(np.float32)
    planar = yuv.planes_to_yuv(planes, fmt="i422", crop=(h, w), out_depth=depth, msb=emsb, siting=siting, **kw)
    want = yuv.pack422(*yuv.split_fmt(planar, "i422"), fmt, depth, msb)
    got = yuv.planes_to_packed(planes, fmt=fmt, crop=(h, w), out_depth=depth, msb=msb, siting=siting, **kw)
    assert got.shape == (B,) + yuv.packed_shape(h, w, fmt) and np.array_equal(got, want)
    if siting == "left":
        assert np.array_equal(yuv.planes_to_packed(planes, fmt=fmt, crop=(h, w), out_depth=depth, msb=msb, siting="topleft", **kw), got)
        assert np.array_equal(yuv.packed_to_planes(frame, fmt=fmt, width=w, depth=depth, msb=msb, siting="topleft", **kw),
                              yuv.packed_to_planes(frame, fmt=fmt, width=w, depth=depth, msb=msb, siting="left", **kw))
        assert not np.array_equal(yuv.planes_to_packed(planes, fmt=fmt, crop=(h, w), out_depth=depth, msb=msb, **kw), got)


def test_definition_refusals():
    z = np.zeros((4, 8), np.uint8)
    with pytest.raises(RuntimeError):
        yuv.packed_to_planes(z, fmt="yuyv")
    with pytest.raises(RuntimeError):
        yuv.packed_to_planes(z, fmt="uyvy", depth=10)
    with pytest.raises(RuntimeError):
        yuv.packed_to_planes(np.zeros((4, 128), np.uint8), fmt="v210", width=6, depth=12)
    with pytest.raises(RuntimeError):
        yuv.packed_shape(4, 5, "uyvy")
    with pytest.raises(RuntimeError):
        yuv.packed_to_planes(z, fmt="uyvy", pad=(0, 4))          # the reflection needs pad < size
    with pytest.raises(RuntimeError):
        yuv.planes_to_packed(np.zeros((1, 3, 4, 6), np.float32), fmt="yuy2", crop=(4, 5))


# ---------------------------------------------------------------------------------------------------- the C ABI, no device
def _surface(lib_mod, **kw):
    f = dict(base=0x10000, pitch=64, bstride=64 * 4, layout=0, depth=8, msb=0)
    f.update(kw)
    return lib_mod.HatPackedSurface(**f)


BAD = {   # name -> (surface fields, call arguments: B, h, w, Hp, Wp, siting)
    "null base": (dict(base=None), {}),
    "odd w": ({}, dict(w=7, Wp=7)),
    "w < 2": ({}, dict(w=0, Wp=0)),
    "h < 1": ({}, dict(h=0, Hp=0)),
    "layout 4": (dict(layout=4), {}),
    "layout -1": (dict(layout=-1), {}),
    "uyvy depth 10": (dict(depth=10), {}),
    "yuy2 depth 16": (dict(layout=1, depth=16), {}),
    "y210 depth 8": (dict(layout=2, depth=8), {}),
    "y210 depth 14": (dict(layout=2, depth=14), {}),
    "v210 depth 12": (dict(layout=3, depth=12, pitch=128, bstride=512), {}),
    "msb 2": (dict(msb=2), {}),
    "siting 3": ({}, dict(siting=3)),
    "siting -1": ({}, dict(siting=-1)),
    "pitch below the row": (dict(pitch=12), {}),
    "v210 pitch below its row quantum": (dict(layout=3, depth=10, pitch=64, bstride=512), {}),
    "base not 4-aligned": (dict(base=0x10002), {}),
    "pitch not 4-aligned": (dict(pitch=66, bstride=66 * 4), {}),
    "y210 base odd": (dict(layout=2, depth=10, base=0x10001), {}),
    "y210 pitch odd": (dict(layout=2, depth=10, pitch=65, bstride=65 * 4), {}),
    "frames overlap": (dict(bstride=64 * 3), {}),
    "bstride not aligned": (dict(bstride=64 * 4 + 2), {}),
}


@pytest.mark.parametrize("name", list(BAD))
def test_entries_refuse_bad_arguments_without_a_device(lib, name):
    from super_resolution_amd import _lib
    fields, args = BAD[name]
    a = dict(B=2, h=4, w=8, Hp=4, Wp=8, siting=0)
    a.update(args)
    s = _surface(_lib, **fields)
    m = (C.c_float * 12)()
    planes = C.c_void_p(0x20000)   # never dereferenced: every case is refused before anything touches a device
    good = _surface(_lib)
    assert lib.hat_packed422_to_planes(C.byref(s), a["siting"], planes, a["B"], a["h"], a["w"], a["Hp"], a["Wp"], m, None) == EINVAL, name
    assert lib.hat_planes_to_packed422(planes, a["B"], 16, 16, C.byref(s), a["siting"], a["h"], a["w"], m, None) == EINVAL, name
    assert good.layout == 0   # (the case differs from an accepted surface in what its name says only)


def test_entries_refuse_null_pointers_and_impossible_reflection(lib):
    from super_resolution_amd import _lib
    s, m, planes = _surface(_lib), (C.c_float * 12)(), C.c_void_p(0x20000)
    to = lambda *a: lib.hat_packed422_to_planes(*a)
    assert to(None, 0, planes, 2, 4, 8, 4, 8, m, None) == EINVAL
    assert to(C.byref(s), 0, None, 2, 4, 8, 4, 8, m, None) == EINVAL
    assert to(C.byref(s), 0, planes, 2, 4, 8, 4, 8, None, None) == EINVAL
    assert to(C.byref(s), 0, planes, 2, 4, 8, 8, 8, m, None) == EINVAL          # Hp - h >= h
    assert to(C.byref(s), 0, planes, 2, 4, 8, 4, 16, m, None) == EINVAL         # Wp - w >= w
    assert to(C.byref(s), 0, planes, 2, 4, 8, 3, 8, m, None) == EINVAL          # Hp < h
    frm = lambda *a: lib.hat_planes_to_packed422(*a)
    assert frm(None, 2, 16, 16, C.byref(s), 0, 4, 8, m, None) == EINVAL
    assert frm(planes, 2, 16, 16, None, 0, 4, 8, m, None) == EINVAL
    assert frm(planes, 2, 16, 16, C.byref(s), 0, 4, 8, None, None) == EINVAL
    assert frm(planes, 2, 3, 16, C.byref(s), 0, 4, 8, m, None) == EINVAL        # the crop does not lie inside the planes
    assert frm(planes, 2, 16, 6, C.byref(s), 0, 4, 8, m, None) == EINVAL
    # the plan entry: a null plan, and before that the rule that a side has exactly one surface
    y = _lib.HatYuvSurface()
    f = lambda sp, ss, dp, ds: lib.hat_plan_forward_packed422(None, sp, ss, 0, dp, ds, 0, 4, 8, m, m, None)
    assert f(C.byref(s), None, C.byref(s), None) == EINVAL


def test_packed_surface_mirror_has_the_c_layout(tmp_path):
    from super_resolution_amd import _lib
    S = _lib.HatPackedSurface
    fields = [f[0] for f in S._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hat_mi355x.h"\nint main(){printf("%zu", sizeof(HatPackedSurface));\n'
    prog += "".join(f'printf(" %zu", offsetof(HatPackedSurface, {f}));\n' for f in fields)
    prog += 'printf(" %d %d %d %d", HAT_PACKED_UYVY, HAT_PACKED_YUY2, HAT_PACKED_Y210, HAT_PACKED_V210);return 0;}\n'
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(S)
    assert vals[1:-4] == [getattr(S, f).offset for f in fields]
    assert vals[-4:] == [yuv.PACKED_FORMATS.index(n) for n in ("uyvy", "yuy2", "y210", "v210")]


def test_uyvy_example_compiles_and_links_with_plain_gcc(lib, tmp_path):
    from super_resolution_amd import build
    exe = tmp_path / "plan_upscale_uyvy"
    libdir = os.path.dirname(build.LIB)
    subprocess.run(["gcc", "-Wall", "-Werror", os.path.join(ROOT, "examples", "plan_upscale_uyvy.c"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + libdir, "-lhat_mi355x", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


# ---------------------------------------------------------------------------------------------------- files
@pytest.mark.parametrize("fmt,depth,msb", [c for c in CASES if c[2] is None], ids=[i for i, c in zip(IDS, CASES) if c[2] is None])
def test_rawvideo_round_trip(fmt, depth, msb, tmp_path):
    h, w = 3, 50
    frames = [yuv.pack422(*_samples(k, h, w, fmt, depth, msb), fmt, depth) for k in range(3)]
    path = str(tmp_path / "clip.raw")
    with rawvideo.Writer(path, fmt, h, w, depth) as wr:
        for f in frames:
            wr.write(f)
        with pytest.raises(rawvideo.RawVideoError):
            wr.write(frames[0][:-1])
    assert os.path.getsize(path) == 3 * frames[0].nbytes
    with rawvideo.Reader(path, fmt, h, w, depth) as rd:
        assert (rd.h, rd.w, rd.depth, rd.fmt) == (h, w, depth, fmt)
        got = list(rd)
    assert len(got) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, frames))
    with open(path, "ab") as f:
        f.write(b"\x00" * 5)
    with rawvideo.Reader(path, fmt, h, w, depth) as rd, pytest.raises(rawvideo.RawVideoError):
        list(rd)


@pytest.mark.parametrize("argv", [["--pixfmt", "uyvy"], ["--pixfmt", "v210", "--raw-size", "4", "6", "--raw-depth", "12"],
                                  ["--raw-size", "4", "6"], ["--pixfmt", "uyvy", "--raw-size", "4", "5"],
                                  ["--out-pixfmt", "v210", "--out-depth", "12"], ["--pixfmt", "nv12", "--raw-size", "4", "6"]],
                         ids=["no size", "v210 depth 12", "size without pixfmt", "odd width", "v210 out depth 12", "no packed layout"])
def test_video_refuses_bad_raw_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        video.parser().parse_args(["-opt", "x.yml", "-i", "in", "-o", "out"] + argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_video_accepts_raw_arguments():
    ns = video.parser().parse_args(["-opt", "x.yml", "-i", "in", "-o", "out", "--pixfmt", "v210", "--raw-size", "4", "6", "--out-pixfmt", "y210",
                                    "--out-depth", "12"])
    assert (ns.pixfmt, ns.raw_size, ns.out_pixfmt, ns.out_depth) == ("v210", [4, 6], "y210", 12)
    ns = video.parser().parse_args(["-opt", "x.yml", "-i", "in.y4m", "-o", "out", "--out-pixfmt", "v210"])
    assert ns.pixfmt is None and ns.out_pixfmt == "v210"
