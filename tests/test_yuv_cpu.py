"""The 4:2:0 frame boundary without a GPU: super_resolution_amd/yuv.py is pinned to the reference's colour conversion
(tests/golden/ycbcr_bt601.npz, written by tests/golden/gen_golden_yuv.py from basicsr/utils/color_util.py) and to the
standards' integer codes; the four new C entries refuse bad arguments before they touch a device; the Y4M reader and writer
are each other's inverse and refuse what they do not support by name; the Y4M example is plain C."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import golden
from super_resolution_amd import y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---------------------------------------------------------------------------------------------- the definition
def test_bt601_is_the_reference_conversion():
    """Bars: the reference works in fp32 on values up to ~300; an fp32 ulp there is 3e-5 in byte units and 1.2e-7 in [0, 1]
    units, with fewer than ten roundings per value: 2e-6 on the input side ([0, 1] units), 1e-4 on the output side (byte
    units).  The reference itself stays inside both against the same constants evaluated in fp64."""
    g = golden("ycbcr_bt601.npz")
    to_rgb, from_rgb = yuv.csc("bt601", False)
    assert to_rgb.dtype == np.float32 and to_rgb.shape == (12,) and from_rgb.dtype == np.float32 and from_rgb.shape == (12,)
    want = np.array([65.481, 128.553, 24.966, 16, -37.797, -74.203, 112.0, 128, 112.0, -93.786, -18.214, 128], dtype=np.float32)
    assert np.array_equal(from_rgb, want), "from_rgb holds the reference's literals"
    ycc, ref = g["ycc"], g["rgb_ref"]
    assert all(len(np.unique(ycc[:, c])) == 256 for c in range(3))
    got = yuv.ycc_to_rgb(ycc[:, 0], ycc[:, 1], ycc[:, 2], to_rgb).T
    assert got.dtype == np.float32
    clipped = float(((ref < 0) | (ref > 1)).mean())
    assert 0.05 < clipped < 0.8, clipped                       # some triples leave [0, 1], most values do not
    e_in = float(np.abs(got.astype(np.float64) - np.clip(ref, 0, 1)).max())
    M = np.array([[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]])   # the same constants in fp64
    rgb_exact = (ycc.astype(np.float64) @ M * 255.0 + np.array([-222.921, 135.576, -276.836])) / 255.0
    e_ref = float(np.abs(np.clip(ref, 0, 1) - np.clip(rgb_exact, 0, 1)).max())
    rgb, ref2 = g["rgb"], g["ycc_ref"]
    Y, cb, cr = yuv.rgb_to_ycc_float(rgb.T[:, None, :], from_rgb)
    pre = np.stack([Y[0], cb[0] + np.float32(128.0), cr[0] + np.float32(128.0)], axis=1)
    e_out = float(np.abs(pre.astype(np.float64) - 255.0 * ref2.astype(np.float64)).max())
    K = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])
    e_ref2 = float(np.abs(255.0 * ref2.astype(np.float64) - (rgb.astype(np.float64) @ K + np.array([16.0, 128.0, 128.0]))).max())
    print(f"input side: yuv.py vs reference {e_in:.3e}, reference vs fp64 {e_ref:.3e}; output side: {e_out:.3e}, {e_ref2:.3e}")
    assert e_ref <= 2e-6 and e_ref2 <= 1e-4, "the reference alone stays inside both bars"
    assert e_in <= 2e-6, e_in
    assert e_out <= 1e-4, e_out


CODES = {  # (matrix, full_range): Y, Cb, Cr of black, white, red, green, blue, mid-grey — the standards' integer codes
    ("bt601", False): [(16, 128, 128), (235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (126, 128, 128)],
    ("bt601", True): [(0, 128, 128), (255, 128, 128), (76, 85, 255), (150, 44, 21), (29, 255, 107), (128, 128, 128)],
    ("bt709", False): [(16, 128, 128), (235, 128, 128), (63, 102, 240), (173, 42, 26), (32, 240, 118), (126, 128, 128)],
    ("bt709", True): [(0, 128, 128), (255, 128, 128), (54, 99, 255), (182, 30, 12), (18, 255, 116), (128, 128, 128)],
}
COLOURS = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5]], dtype=np.float32)


@pytest.mark.parametrize("key", list(CODES), ids=[f"{m}_{'full' if f else 'limited'}" for m, f in CODES])
def test_known_answers(key):
    """0.5 grey is 125.5 (limited) / 127.5 (full) before rounding: half to even gives 126 / 128."""
    matrix, full = key
    planes = np.repeat(np.repeat(COLOURS.T[None, :, None, :], 2, axis=2), 2, axis=3)     # (1,3,2,12): one 2 x 2 block per colour
    for fmt in yuv.FORMATS:
        frame = yuv.planes_to_yuv420(planes, fmt=fmt, matrix=matrix, full_range=full)
        assert frame.shape == (1, 3, 12) and frame.dtype == np.uint8
        Y, Cb, Cr = yuv.split(frame, fmt)
        got = [(int(Y[0, 0, 2 * i]), int(Cb[0, 0, i]), int(Cr[0, 0, i])) for i in range(6)]
        assert got == CODES[key], (fmt, got)
        assert (Y[0, 0] == Y[0, 1]).all()
        back = yuv.yuv420_to_planes(frame, fmt=fmt, matrix=matrix, full_range=full)
        assert back.shape == planes.shape and back.dtype == np.float32
        tol = 1.5 / 219 if not full else 1.5 / 255                                       # the codes are rounded: within 1.5 code steps
        # black and white come back exactly but for the constants' own rounding: the reference's inverse has six digits
        # (0.5e-8 x (235 + 112 + 112) = 2.3e-6 and an offset rounded at 1e-3 / 255 = 2e-6), the derived ones are fp32 (1e-7 x 4)
        assert np.abs(back[:, :, :, :4] - planes[:, :, :, :4]).max() <= 5e-6
        assert np.abs(back - planes).max() <= 3 * tol


@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_host_round_trip_and_layouts(fmt):
    rng = np.random.default_rng(3)
    B, h, w = 2, 12, 20
    Y = np.repeat(np.repeat(rng.integers(90, 160, (B, h // 2, w // 2), dtype=np.uint8), 2, 1), 2, 2)     # constant per 2 x 2 block, mid-range
    Cb, Cr = rng.integers(100, 156, (2, B, h // 2, w // 2), dtype=np.uint8)    # near grey: every triple lies inside the RGB cube
    f = yuv.join(Y, Cb, Cr, fmt)
    assert f.shape == (B, 18, 20)
    y2, cb2, cr2 = yuv.split(f, fmt)
    assert np.array_equal(y2, Y) and np.array_equal(cb2, Cb) and np.array_equal(cr2, Cr)
    raw = f[0].reshape(-1)
    assert np.array_equal(raw[:h * w], Y[0].reshape(-1))
    if fmt == "i420":
        assert np.array_equal(raw[h * w:h * w + h * w // 4], Cb[0].reshape(-1)) and np.array_equal(raw[h * w + h * w // 4:], Cr[0].reshape(-1))
    else:
        a, b = (Cb, Cr) if fmt == "nv12" else (Cr, Cb)
        assert np.array_equal(raw[h * w::2], a[0].reshape(-1)) and np.array_equal(raw[h * w + 1::2], b[0].reshape(-1))
    planes = yuv.yuv420_to_planes(f, fmt=fmt)
    assert planes.min() > 0 and planes.max() < 1, "no triple of this frame is clipped"
    back = yuv.planes_to_yuv420(planes, fmt=fmt)
    assert np.abs(back.astype(int) - f.astype(int)).max() <= 1
    padded = yuv.yuv420_to_planes(f, fmt=fmt, pad=(4, 6))                       # F.pad 'reflect' on the bottom and the right
    assert padded.shape == (B, 3, 16, 26)
    assert np.array_equal(padded[:, :, :h, :w], planes)
    assert np.array_equal(padded[:, :, h:, :w], planes[:, :, h - 2:h - 6:-1]) and np.array_equal(padded[:, :, :h, w:], planes[:, :, :, w - 2:w - 8:-1])
    assert np.array_equal(yuv.yuv420_to_planes(f[0], fmt=fmt), planes[:1])     # a frame without the batch axis


def test_yuv_refusals():
    with pytest.raises(RuntimeError, match="even"):
        yuv.yuv420_to_planes(np.zeros((15, 9), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="even"):
        yuv.planes_to_yuv420(np.zeros((1, 3, 8, 8), dtype=np.float32), crop=(7, 8))
    with pytest.raises(RuntimeError, match="format"):
        yuv.yuv420_to_planes(np.zeros((12, 8), dtype=np.uint8), fmt="yuyv")
    with pytest.raises(RuntimeError, match="matrix"):
        yuv.csc("bt2020")
    with pytest.raises(RuntimeError, match="smaller"):
        yuv.yuv420_to_planes(np.zeros((12, 8), dtype=np.uint8), pad=(8, 0))


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


def test_yuv420_to_planes_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem)
    ok = dict(y=p, y_pitch=20, y_bstride=20 * 10, cb=p, cr=p, c_pitch=20, c_step=2, c_bstride=20 * 5, dst=p, B=1, h=10, w=20, Hp=16, Wp=32,
              m=_m12())
    call = lambda **kw: lib.hat_yuv420_to_planes(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("y", "cb", "cr", "dst", "m"):
        assert call(**{k: None}) == EINVAL, k
    assert call(B=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(h=9) == EINVAL and call(w=19) == EINVAL                      # odd sizes
    assert call(c_step=0) == EINVAL and call(c_step=3) == EINVAL
    assert call(y_pitch=19) == EINVAL                                        # y_pitch < w
    assert call(c_pitch=19) == EINVAL and call(c_step=1, c_pitch=9) == EINVAL   # c_pitch < c_step w / 2
    assert call(Hp=8) == EINVAL and call(Wp=18) == EINVAL                    # the padded plane is smaller than the frame
    assert call(Hp=20) == EINVAL and call(Wp=40) == EINVAL                   # padding == size: nothing left to reflect
    assert call(B=2, y_bstride=20 * 9) == EINVAL and call(B=2, c_bstride=20 * 4) == EINVAL   # samples overlap


def test_planes_to_yuv420_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem)
    ok = dict(src=p, B=1, Hs=16, Ws=32, y=p, y_pitch=30, y_bstride=30 * 12, cb=p, cr=p, c_pitch=15, c_step=1, c_bstride=15 * 6, h=12, w=30,
              m=_m12())
    call = lambda **kw: lib.hat_planes_to_yuv420(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("src", "y", "cb", "cr", "m"):
        assert call(**{k: None}) == EINVAL, k
    assert call(B=0) == EINVAL and call(Hs=0) == EINVAL and call(Ws=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(h=11) == EINVAL and call(w=29) == EINVAL
    assert call(c_step=0) == EINVAL and call(c_step=3) == EINVAL
    assert call(y_pitch=29) == EINVAL and call(c_pitch=14) == EINVAL and call(c_step=2, c_pitch=29) == EINVAL
    assert call(h=18) == EINVAL and call(w=34, y_pitch=34, c_pitch=17) == EINVAL   # crop larger than the source
    assert call(B=2, y_bstride=30 * 11) == EINVAL and call(B=2, c_bstride=15 * 5) == EINVAL


def test_conv3x3_to_yuv420_rejects_bad_arguments(lib, mem):
    from super_resolution_amd import _lib
    p = C.addressof(mem) // 16 * 16 + 16
    mean = (C.c_float * 4)(0.4488, 0.4371, 0.4040, 0.0)
    ok = dict(x=p, wpk=p, bias=p, y=p, y_pitch=30, y_bstride=30 * 12, cb=p, cr=p, c_pitch=30, c_step=2, c_bstride=30 * 6, B=1, H=16, W=32, Cc=64,
              ldx=64, h=12, w=30, scale=1.0, mean=mean, m=_m12(), dtype=_lib.HAT_BF16)
    call = lambda **kw: lib.hat_conv3x3_to_yuv420(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("x", "wpk", "bias", "y", "cb", "cr", "mean", "m"):
        assert call(**{k: None}) == EINVAL, k
    assert call(B=0) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(W=40) == EINVAL                                              # the row sweep needs W % 16 == 0
    assert call(h=11) == EINVAL and call(w=29) == EINVAL
    assert call(c_step=0) == EINVAL and call(c_step=3) == EINVAL
    assert call(y_pitch=29) == EINVAL and call(c_pitch=29) == EINVAL and call(c_step=1, c_pitch=14) == EINVAL
    assert call(h=18) == EINVAL and call(w=34, y_pitch=34, c_pitch=34) == EINVAL
    assert call(B=2, y_bstride=30 * 11) == EINVAL
    assert call(x=p + 2) == EINVAL                                           # fragment loads are 16-byte aligned
    assert call(dtype=_lib.HAT_F32) == -3 and call(Cc=48) == -3               # HAT_EUNSUPPORTED: only the bf16 conv_last shape is built


def test_plan_forward_yuv420_rejects_bad_arguments(lib, mem):
    """What needs no plan is checked before the plan is read (a stand-in handle is never dereferenced); the checks against
    the plan's shape are tests/test_gpu_yuv.py::test_plan_forward_yuv420's."""
    p = C.addressof(mem)
    ok = dict(plan=p, sy=p, sy_pitch=20, sy_bs=0, scb=p, scr=p, sc_pitch=10, sc_step=1, sc_bs=0, h=10, w=20,
              dy=p, dy_pitch=40, dy_bs=0, dcb=p, dcr=p, dc_pitch=20, dc_step=1, dc_bs=0, to=_m12(), fr=_m12())
    call = lambda **kw: lib.hat_plan_forward_yuv420(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("plan", "sy", "scb", "scr", "dy", "dcb", "dcr", "to", "fr"):
        assert call(**{k: None}) == EINVAL, k
    assert call(h=0) == EINVAL and call(w=0) == EINVAL and call(h=9) == EINVAL and call(w=19) == EINVAL
    assert call(sc_step=0) == EINVAL and call(sc_step=3) == EINVAL and call(dc_step=0) == EINVAL and call(dc_step=3) == EINVAL
    assert call(sy_pitch=19) == EINVAL and call(sc_pitch=9) == EINVAL and call(sc_step=2, sc_pitch=19) == EINVAL


# ---------------------------------------------------------------------------------------------- Y4M
def _frames(seed, n, h, w):
    return [np.random.default_rng(seed + i).integers(0, 256, (3 * h // 2, w), dtype=np.uint8) for i in range(n)]


def test_y4m_writer_then_reader_is_the_identity(tmp_path):
    hdr = {"W": 22, "H": 14, "F": "30000:1001", "I": "p", "A": "1:1", "C": "420mpeg2", "X": ["YSCSS=420MPEG2", "COLORRANGE=LIMITED"]}
    frames = _frames(1, 3, 14, 22)
    path = tmp_path / "a.y4m"
    with y4m.Writer(str(path), hdr) as wr:
        for f in frames:
            wr.write(f)
    raw = path.read_bytes()
    assert raw.startswith(b"YUV4MPEG2 W22 H14 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\nFRAME\n")
    assert len(raw) == raw.index(b"\n") + 1 + 3 * (6 + 22 * 14 * 3 // 2)
    with y4m.Reader(str(path)) as rd:
        assert rd.header == hdr and (rd.w, rd.h) == (22, 14)
        got = list(rd)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))
    # a header without optional tokens, FRAME records with parameters, a file object instead of a path
    buf = io.BytesIO(b"YUV4MPEG2 W4 H2\nFRAME Ip\n" + bytes(range(12)) + b"FRAME\n" + bytes(range(12, 24)))
    rd = y4m.Reader(buf)
    assert rd.header == {"W": 4, "H": 2, "X": []}
    a, b = list(rd)
    assert a.shape == (3, 4) and a.reshape(-1).tolist() == list(range(12)) and b.reshape(-1).tolist() == list(range(12, 24))
    for c in ("420", "420jpeg", "420mpeg2", "420paldv"):
        assert y4m.parse_header(b"YUV4MPEG2 W4 H2 C" + c.encode())["C"] == c


def test_y4m_refusals(tmp_path):
    with pytest.raises(y4m.Y4MError, match="C444"):
        y4m.parse_header(b"YUV4MPEG2 W4 H4 C444")
    with pytest.raises(y4m.Y4MError, match="C420p10.*8 bits"):
        y4m.parse_header(b"YUV4MPEG2 W4 H4 C420p10")
    with pytest.raises(y4m.Y4MError, match="even.*W5"):
        y4m.parse_header(b"YUV4MPEG2 W5 H4 C420")
    with pytest.raises(y4m.Y4MError, match="YUV4MPEG2"):
        y4m.parse_header(b"P6 4 4 255")
    rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H2 C420jpeg\nFRAME\n" + bytes(11)))
    with pytest.raises(y4m.Y4MError, match="truncated"):
        next(rd)
    with pytest.raises(y4m.Y4MError, match="FRAME"):
        next(y4m.Reader(io.BytesIO(b"YUV4MPEG2 W4 H2\nFRAMF\n" + bytes(12))))
    with pytest.raises(y4m.Y4MError, match="C422"):
        y4m.Writer(io.BytesIO(), {"W": 4, "H": 2, "C": "422"})
    wr = y4m.Writer(io.BytesIO(), {"W": 4, "H": 2})
    with pytest.raises(y4m.Y4MError, match="frame"):
        wr.write(np.zeros((2, 4), dtype=np.uint8))


def test_video_header_arithmetic():
    hdr = y4m.parse_header(b"YUV4MPEG2 W1280 H720 F25:1 It A1:1 C420paldv XFOO")
    out = y4m.scaled_header(hdr, 4)
    assert out == {"W": 5120, "H": 2880, "F": "25:1", "I": "t", "A": "1:1", "C": "420paldv", "X": ["FOO"]}
    assert y4m.format_header(out) == b"YUV4MPEG2 W5120 H2880 F25:1 It A1:1 C420paldv XFOO\n"
    assert hdr["W"] == 1280 and out["X"] is not hdr["X"]


def test_video_file_loop_and_command_line(tmp_path, monkeypatch):
    """upscale_file with the device part replaced: a stand-in for frames.upscale_frames that repeats every sample s times in both
    directions (which keeps a (3h/2, w) array a valid i420 frame of the scaled size) and records how it was called."""
    from super_resolution_amd import frames, video
    hdr = {"W": 6, "H": 4, "F": "24:1", "I": "p", "A": "1:1", "C": "420jpeg", "X": ["NOTE"]}
    seq = _frames(9, 3, 4, 6)
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr) as wr:
        for f in seq:
            wr.write(f)
    calls = []

    class Net:
        upscale = 3

    def fake(net, it, **kw):
        calls.append(kw)
        for a in it:
            yield np.repeat(np.repeat(a, net.upscale, 0), net.upscale, 1)

    monkeypatch.setattr(frames, "upscale_frames", fake)
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), matrix="bt709", full_range=True)
    assert info == {"frames": 3, "in": (6, 4), "out": (18, 12)}
    assert calls == [{"pixfmt": "i420", "matrix": "bt709", "full_range": True}]
    with y4m.Reader(str(tmp_path / "out.y4m")) as rd:
        assert rd.header == dict(hdr, W=18, H=12)
        got = list(rd)
    assert len(got) == 3 and all(np.array_equal(g, np.repeat(np.repeat(a, 3, 0), 3, 1)) for g, a in zip(got, seq))
    args = video.parser().parse_args(["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m"])
    assert (args.opt, args.input, args.output, args.matrix, args.full_range, args.device) == ("o.yml", "a.y4m", "b.y4m", "bt601", False, "cuda:0")
    args = video.parser().parse_args(["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m", "--matrix", "bt709", "--full-range"])
    assert (args.matrix, args.full_range) == ("bt709", True)
    with pytest.raises(SystemExit):
        video.parser().parse_args(["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m", "--matrix", "bt2020"])
    with pytest.raises(SystemExit):
        video.parser().parse_args(["-i", "a.y4m", "-o", "b.y4m"])


def test_y4m_example_is_plain_c(tmp_path):
    """examples/plan_upscale_y4m.c compiles as C (not C++) and links against the library and the HIP runtime with gcc alone;
    its matrices are yuv.csc()'s."""
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
    assert os.path.exists(exe)
    import re
    text = open(src).read()
    for name, want in zip(("TO_RGB", "FROM_RGB"), yuv.csc()):
        body = re.search(name + r"\[12\] = \{(.*?)\};", text, re.S).group(1)
        vals = np.array([float(v.strip().rstrip("f")) for v in body.split(",")], dtype=np.float32)
        assert np.array_equal(vals, want), name
