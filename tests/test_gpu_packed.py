"""Packed 4:2:2 (UYVY / YUY2 / Y210 / v210) on the GPU: the two kernels, the models' frame calls, the frame generator, the plans and the C
example.  Every comparison is an equality — with the definition (super_resolution_amd/yuv.py: packed_to_planes / planes_to_packed,
which ARE the 'i422' functions on the unpacked samples) and with the planar 'i422' kernels and calls of the same build, repacked on
the host: a packed sample goes through the expressions of a (1, 0) surface, so there is no tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import META, W_SEED
from super_resolution_amd import synth, yuv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("uyvy", 8, None), ("yuy2", 8, None), ("y210", 10, None), ("y210", 10, False), ("y210", 16, None), ("v210", 10, None)]
IDS = ["uyvy", "yuy2", "y210msb", "y210lsb", "y216", "v210"]
CSC = [dict(matrix="bt601", full_range=False), dict(matrix="bt709", full_range=True)]
WIDTHS = (2, 6, 8, 46, 48, 50)     # a pair; one v210 group; a partial group; both sides of the 48-pixel row quantum
HEIGHTS = (1, 3)
B = 2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _net(arch, name, dtype, dev):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(type=arch, compute_dtype=dtype, **META["cfgs"][name])).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    return net.to(dev)


def _t(a, dev):
    """numpy frames -> device tensor (uint16 goes through int16: the same words)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(dev) if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)


def _n(t):
    a = t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)
    return np.ascontiguousarray(a)


def _frame(seed, lead, h, w, fmt, depth, msb):
    """A random packed frame: every byte / word value (LSB words above the code range saturate, MSB words carry low bits); v210 from
    random codes, with garbage in the bits and bytes that are not read."""
    rng = np.random.default_rng(seed)
    if fmt != "v210":
        dt = yuv.packed_container(fmt, depth, msb)[0]
        return rng.integers(0, 256 if dt is np.uint8 else 65536, lead + yuv.packed_shape(h, w, fmt)).astype(dt)
    f = yuv.pack422(*(rng.integers(0, 1024, lead + (h, n)).astype(np.uint16) for n in (w, w // 2, w // 2)), "v210")
    f.view("<u4")[...] |= np.uint32(0xC0000000)
    f[..., 16 * -(-w // 6):] = 0xA5
    return f


def _pitched(frame, dev, fill=0):
    """The device copy of (B, h, row) frames as a view of a larger tensor: rows one unit longer, one more row a frame, so the pitch
    and the batch stride are larger than the frame's.  -> (view, the whole tensor)."""
    Bn, h, row = frame.shape
    unit = 4                                                       # elements: 4 bytes (8-bit, v210), 8 bytes (y210), a unit each
    tdt = torch.uint8 if frame.dtype == np.uint8 else torch.int16
    big = torch.full((Bn, h + 1, row + unit), fill, dtype=tdt, device=dev)
    big[:, :h, :row] = torch.from_numpy(np.ascontiguousarray(frame).view(np.uint8 if tdt is torch.uint8 else np.int16)).to(dev)
    big = big if tdt is torch.uint8 else big.view(torch.uint16)
    return big[:, :h, :row], big


def _twin(frame, fmt, depth, msb, w):
    """The 'i422' frame with the samples of a packed frame, and the alignment its words have."""
    emsb = yuv.packed_container(fmt, depth, msb)[2]
    return yuv.join_fmt(*yuv.unpack422(frame, fmt, w, depth, msb), "i422", depth, emsb), emsb


def _repack(planar, fmt, depth, msb):
    return yuv.pack422(*yuv.split_fmt(planar, "i422"), fmt, depth, msb)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("csc", CSC, ids=["bt601", "bt709full"])
@pytest.mark.parametrize("siting", ["center", "left"])
@pytest.mark.parametrize("fmt,depth,msb", CASES, ids=IDS)
def test_packed422_to_planes_equals_the_definition(fmt, depth, msb, siting, csc):
    """Every width and height, the largest reflection the frame allows and none, pitched rows and frames; and the planar i422
    kernel on the unpacked samples gives the same planes (device = device)."""
    dev = _dev()
    from super_resolution_amd import ops
    to_rgb = yuv.csc(depth=depth, **csc)[0]
    for h in HEIGHTS:
        for w in WIDTHS:
            frame = _frame(h * 100 + w, (B,), h, w, fmt, depth, msb)
            src, _keep = _pitched(frame, dev)
            for pad in ((h - 1, w - 1), (0, 0)):
                want = yuv.packed_to_planes(frame, fmt=fmt, width=w, depth=depth, msb=msb, pad=pad, siting=siting, **csc)
                got = torch.full((B, 3, h + pad[0], w + pad[1]), float("nan"), device=dev)
                ops.packed422_to_planes(src, got, to_rgb, fmt=fmt, width=w, depth=depth, msb=msb, siting=siting)
                assert np.array_equal(got.cpu().numpy(), want), f"{fmt} {h}x{w} pad {pad} {siting}"
            planar, emsb = _twin(frame, fmt, depth, msb, w)
            dd = torch.full((B, 3, 2 * h - 1, 2 * w - 1), float("nan"), device=dev)
            ops.yuv_to_planes(*ops.yuv_views(_t(planar, dev), "i422"), dd, to_rgb, sub=(1, 0), depth=depth, msb=emsb, siting=siting)
            got = torch.empty_like(dd)
            ops.packed422_to_planes(src, got, to_rgb, fmt=fmt, width=w, depth=depth, msb=msb, siting=siting)
            assert torch.equal(got, dd), f"{fmt} {h}x{w} {siting}: differs from the planar i422 kernel"


@pytest.mark.parametrize("csc", CSC, ids=["bt601", "bt709full"])
@pytest.mark.parametrize("siting", ["center", "left"])
@pytest.mark.parametrize("fmt,depth,msb", CASES, ids=IDS)
def test_planes_to_packed422_equals_the_definition(fmt, depth, msb, siting, csc):
    """Planes larger than the crop, a destination filled with 99 whose pitched rows and frames keep their 99 past the layout's row,
    v210's zero tail and top bits; and the planar i422 kernel's samples on the same planes, repacked on the host, are the same."""
    dev = _dev()
    from super_resolution_amd import ops
    from_rgb = yuv.csc(depth=depth, **csc)[1]
    for h in HEIGHTS:
        for w in WIDTHS:
            planes = np.random.default_rng(h * 100 + w).uniform(-0.2, 1.2, (B, 3, h + 1, w + 3)).astype(np.float32)
            want = yuv.planes_to_packed(planes, fmt=fmt, crop=(h, w), out_depth=depth, msb=msb, siting=siting, **csc)
            dst, big = _pitched(np.full(want.shape, 99, want.dtype), dev, fill=99)
            p = torch.from_numpy(planes).to(dev)
            ops.planes_to_packed422(p, dst, from_rgb, fmt=fmt, width=w, depth=depth, msb=msb, siting=siting)
            got, whole = _n(dst), _n(big)
            assert np.array_equal(got, want), f"{fmt} {h}x{w} {siting}"
            row = want.shape[2]
            assert (whole[:, :h, row:] == 99).all() and (whole[:, h:] == 99).all(), f"{fmt} {h}x{w}: wrote past the layout's row"
            if fmt == "v210":
                assert not (got.view("<u4") >> 30).any() and not got[:, :, 16 * -(-w // 6):].any()
            emsb = yuv.packed_container(fmt, depth, msb)[2]
            planar = torch.zeros((B,) + yuv.frame_shape_fmt(h, w, "i422"), dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
            planar = planar if depth == 8 else planar.view(torch.uint16)
            ops.planes_to_yuv(p, *ops.yuv_views(planar, "i422"), from_rgb, sub=(1, 0), depth=depth, msb=emsb, siting=siting)
            assert np.array_equal(_repack(_n(planar), fmt, depth, msb), got), f"{fmt} {h}x{w} {siting}: differs from the planar i422 kernel"


def test_topleft_is_left_and_wrappers_refuse():
    dev = _dev()
    from super_resolution_amd import ops
    frame = _frame(1, (B,), 3, 8, "uyvy", 8, None)
    a, b = (torch.empty(B, 3, 4, 12, device=dev) for _ in range(2))
    ops.packed422_to_planes(_t(frame, dev), a, yuv.csc()[0], fmt="uyvy", siting="left")
    ops.packed422_to_planes(_t(frame, dev), b, yuv.csc()[0], fmt="uyvy", siting="topleft")
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.packed422_to_planes(torch.zeros(B, 3, 128, dtype=torch.uint8, device=dev), a, yuv.csc()[0], fmt="v210", depth=10)
    with pytest.raises(TypeError):
        ops.packed422_to_planes(torch.zeros(B, 3, 16, dtype=torch.uint8, device=dev), a, yuv.csc()[0], fmt="y210", depth=10)
    with pytest.raises(RuntimeError):
        ops.packed422_to_planes(_t(frame, dev), torch.empty(B, 3, 6, 8, device=dev), yuv.csc()[0], fmt="uyvy")   # no such reflection


# ---------------------------------------------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def tiny():
    return _net("HAT", "tiny_x3", "bf16", _dev())


@pytest.mark.parametrize("fmt,depth,msb", [c for c in CASES if c[2] is None and c[1] != 16], ids=["uyvy", "yuy2", "y210", "v210"])
def test_forward_yuv_equals_the_i422_forward_repacked(tiny, fmt, depth, msb):
    """13 x 22 frames pad to 16 x 24 (window 8); left-sited on both sides, as standard 4:2:2 is, and centre-sited."""
    dev = _dev()
    h, w = 13, 22
    frame = _frame(7, (B,), h, w, fmt, depth, msb)
    planar, emsb = _twin(frame, fmt, depth, msb, w)
    before = tiny.engine(dev).yuv_planes_calls
    for siting in ("left", "center"):
        want = _repack(_n(tiny.forward_yuv(_t(planar, dev), fmt="i422", depth=depth, msb=emsb, out_msb=emsb, siting=siting)), fmt, depth, msb)
        planes_calls = tiny.engine(dev).yuv_planes_calls
        got = tiny.forward_yuv(_t(frame, dev), fmt=fmt, depth=depth, siting=siting, width=w)
        assert tiny.engine(dev).yuv_planes_calls == planes_calls + 1          # a packed output always ends in planes
        assert tuple(got.shape) == (B,) + yuv.packed_shape(3 * h, 3 * w, fmt)
        assert np.array_equal(_n(got), want), f"{fmt} {siting}"
    assert tiny.engine(dev).yuv_planes_calls > before


def test_forward_yuv_mixes_packed_and_planar_sides(tiny):
    dev = _dev()
    h, w = 12, 22
    nv12 = np.random.default_rng(3).integers(0, 256, (B,) + yuv.frame_shape_fmt(h, w, "nv12")).astype(np.uint8)
    want = _repack(_n(tiny.forward_yuv(_t(nv12, dev), fmt="nv12", out_fmt="i422", out_depth=10, out_msb=False, siting="left")), "v210", 10, None)
    got = tiny.forward_yuv(_t(nv12, dev), fmt="nv12", out_fmt="v210", out_depth=10, siting="left")
    assert np.array_equal(_n(got), want)
    uyvy = _frame(4, (B,), h, w, "uyvy", 8, None)
    planar, _ = _twin(uyvy, "uyvy", 8, None, w)
    want = tiny.forward_yuv(_t(planar, dev), fmt="i422", out_fmt="i420")
    fused = tiny.engine(dev).yuv_fused_calls
    got = tiny.forward_yuv(_t(uyvy, dev), fmt="uyvy", out_fmt="i420")
    assert torch.equal(got, want)
    # 16 x 24 frames have wd = 72, no multiple of 16: tiny_x3's planar outputs go through planes here; the counters say which
    assert tiny.engine(dev).yuv_fused_calls >= fused


def test_forward_yuv_ensemble_out_and_refusals(tiny):
    dev = _dev()
    h, w = 13, 22
    frame = _frame(9, (B,), h, w, "yuy2", 8, None)
    planar, _ = _twin(frame, "yuy2", 8, None, w)
    want = _repack(_n(tiny.forward_yuv(_t(planar, dev), fmt="i422", ensemble=2)), "yuy2", 8, None)
    assert np.array_equal(_n(tiny.forward_yuv(_t(frame, dev), fmt="yuy2", ensemble=2)), want)
    v = _frame(10, (B,), h, w, "v210", 10, None)
    out = torch.full((B,) + yuv.packed_shape(3 * h, 3 * w, "v210"), 99, dtype=torch.uint8, device=dev)
    ret = tiny.forward_yuv(_t(v, dev), fmt="v210", depth=10, width=w, out=out)
    assert ret is out
    pv, _ = _twin(v, "v210", 10, None, w)
    assert np.array_equal(_n(out), _repack(_n(tiny.forward_yuv(_t(pv, dev), fmt="i422", depth=10, msb=False, out_msb=False)), "v210", 10, None))
    with pytest.raises(ValueError):
        tiny.forward_yuv(_t(v, dev), fmt="v210", depth=10)                      # no width
    with pytest.raises(ValueError):
        tiny.forward_yuv(_t(frame, dev), fmt="yuy2", width=w + 2)               # optional and checked
    with pytest.raises(RuntimeError):
        tiny.forward_yuv(_t(v, dev), fmt="v210", depth=12, width=w)
    with pytest.raises(TypeError):
        tiny.forward_yuv(_t(frame, dev), fmt="y210", depth=10)
    with pytest.raises(RuntimeError):
        tiny.forward_yuv(_t(frame, dev), fmt="yuy2", out=out)
    with pytest.raises(RuntimeError):
        tiny.forward_yuv420(_t(frame, dev), fmt="uyvy")                          # keeps to its three layouts


def test_esc_upscale_yuv_uyvy():
    from test_gpu_esc import _net as esc_net
    dev = _dev()
    net, g, _ = esc_net("a", "bf16", dev)
    h, w = int(g["x"].shape[2]), int(g["x"].shape[3]) & ~1
    frame = _frame(11, (1,), h, w, "uyvy", 8, None)
    planar, _ = _twin(frame, "uyvy", 8, None, w)
    want = _repack(_n(net.upscale_yuv(_t(planar, dev), fmt="i422", siting="left")), "uyvy", 8, None)
    assert np.array_equal(_n(net.upscale_yuv(_t(frame, dev), fmt="uyvy", siting="left")), want)


def test_esclte_upscale_yuv_y210_to_an_odd_ratio_size():
    from test_gpu_esclte import _net as lte_net
    dev = _dev()
    net, _, _ = lte_net("a", "bf16")
    h, w, size = 20, 24, (31, 42)                                               # x1.55, x1.75
    frame = _frame(12, (1,), h, w, "y210", 10, None)
    planar, emsb = _twin(frame, "y210", 10, None, w)
    want = _repack(_n(net.upscale_yuv(_t(planar, dev), size=size, fmt="i422", depth=10, msb=emsb, out_msb=emsb, out_siting="left")), "y210", 10, None)
    got = net.upscale_yuv(_t(frame, dev), size=size, fmt="y210", depth=10, out_siting="left")
    assert tuple(got.shape) == (1,) + yuv.packed_shape(*size, "y210") and np.array_equal(_n(got), want)
    with pytest.raises(ValueError):
        net.upscale_yuv(_t(frame, dev), size=(31, 41), fmt="y210", depth=10)


def test_upscale_frames_uyvy_in_order(tiny):
    dev = _dev()
    from super_resolution_amd import frames as FR
    seq = [_frame(20 + i, (), 13, 22, "uyvy", 8, None) for i in range(3)]
    got = list(FR.upscale_frames(tiny, iter(seq), pixfmt="uyvy", siting="left"))
    assert len(got) == 3
    for g, f in zip(got, seq):
        assert np.array_equal(g, _n(tiny.forward_yuv(_t(f[None], dev), fmt="uyvy", siting="left"))[0])
    assert FR.PIXFMTS[-4:] == yuv.PACKED_FORMATS


# ---------------------------------------------------------------------------------------------------- plans and the C example
def test_plan_forward_packed422(tmp_path):
    dev = _dev()
    from super_resolution_amd import _lib, ops, plan
    net = _net("HAT", "tiny_x3", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (B, 3, 16, 24), path)
    p = plan.Plan(path)
    h, w = 13, 22
    uyvy = _t(_frame(30, (B,), h, w, "uyvy", 8, None), dev)
    dst = torch.full((B,) + yuv.packed_shape(3 * h, 3 * w, "uyvy"), 99, dtype=torch.uint8, device=dev)
    p.forward_yuv(uyvy, dst, fmt="uyvy", siting="left")
    torch.cuda.synchronize()
    assert torch.equal(dst, net.forward_yuv(uyvy, fmt="uyvy", siting="left"))
    nv12 = _t(np.random.default_rng(31).integers(0, 256, (B,) + yuv.frame_shape_fmt(12, w, "nv12")).astype(np.uint8), dev)
    dv = torch.full((B,) + yuv.packed_shape(36, 3 * w, "v210"), 99, dtype=torch.uint8, device=dev)
    p.forward_yuv(nv12, dv, fmt="nv12", out_fmt="v210", out_depth=10)
    torch.cuda.synchronize()
    assert torch.equal(dv, net.forward_yuv(nv12, fmt="nv12", out_fmt="v210", out_depth=10))
    i420 = torch.empty((B,) + yuv.frame_shape_fmt(36, 3 * w, "i420"), dtype=torch.uint8, device=dev)
    uy12 = _t(_frame(32, (B,), 12, w, "uyvy", 8, None), dev)
    p.forward_yuv(uy12, i420, fmt="uyvy", out_fmt="i420")
    torch.cuda.synchronize()
    assert torch.equal(i420, net.forward_yuv(uy12, fmt="uyvy", out_fmt="i420"))
    # a side has exactly one surface
    sp = ops.packed_surface(uyvy, "uyvy")[0]
    dp = ops.packed_surface(dst, "uyvy")[0]
    ys = ops.yuv_surface(*ops.yuv_views(i420, "i420"), sub=(1, 1))
    m = ops._f12(yuv.csc()[0])
    f = lambda a, b, c, d: p._lib.hat_plan_forward_packed422(p._h, a, b, 0, c, d, 0, h, w, m, m, 0)
    ref = C.byref
    assert f(None, None, ref(dp), None) == -1 and f(ref(sp), ref(ys), ref(dp), None) == -1
    assert f(ref(sp), None, None, None) == -1 and f(ref(sp), None, ref(dp), ref(ys)) == -1
    p.close()


def test_c_example_equals_the_file_tool(tmp_path):
    dev = _dev()
    from super_resolution_amd import plan, rawvideo, video
    exe = tmp_path / "plan_upscale_uyvy"
    lib = os.path.join(ROOT, "super_resolution_amd")
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_uyvy.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + lib, "-lhat_mi355x", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    net = _net("HAT", "tiny_x3", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 16, 24), path)
    h, w = 13, 22
    with rawvideo.Writer(str(tmp_path / "in.uyvy"), "uyvy", h, w) as wr:
        for i in range(3):
            wr.write(_frame(40 + i, (), h, w, "uyvy", 8, None))
    info = video.upscale_file(net, str(tmp_path / "in.uyvy"), str(tmp_path / "py.uyvy"), pixfmt="uyvy", raw_size=(h, w), out_pixfmt="uyvy",
                              chroma_loc="left")
    assert info["frames"] == 3 and info["out"] == (3 * w, 3 * h)
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, "--size", str(h), str(w), str(tmp_path / "in.uyvy"), str(tmp_path / "c.uyvy"),
                        "--left"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = open(tmp_path / "py.uyvy", "rb").read(), open(tmp_path / "c.uyvy", "rb").read()
    assert len(a) == 3 * 2 * 9 * h * w and a == b
    # Y4M in, v210 out: the side without its flag is Y4M
    from super_resolution_amd import y4m
    with y4m.Writer(str(tmp_path / "in.y4m"), {"W": w, "H": 12, "F": "25:1", "C": "420jpeg", "X": []}, chroma=True) as wr:
        f420 = np.random.default_rng(5).integers(0, 256, yuv.frame_shape_fmt(12, w, "i420")).astype(np.uint8)
        wr.write(f420)
    info = video.upscale_file(net, str(tmp_path / "in.y4m"), str(tmp_path / "out.v210"), out_pixfmt="v210")
    assert info["out_depth"] == 10 and info["frames"] == 1
    with rawvideo.Reader(str(tmp_path / "out.v210"), "v210", 36, 3 * w) as rd:
        got = list(rd)
    assert len(got) == 1 and np.array_equal(got[0], _n(net.forward_yuv(_t(f420[None], dev), fmt="i420", out_fmt="v210", out_depth=10))[0])
