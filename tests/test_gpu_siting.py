"""Chroma siting on the GPU: the co-sited instances of the two surface kernels, forward_yuv with siting= / out_siting=, the plans, the C
example and the file tool.  Every comparison with the definition (super_resolution_amd/yuv.py, "Chroma siting", pinned by hand-written
values in tests/test_siting_cpu.py) is an equality: the input interpolation is exact in fp32, and every sum of the output taps is
rounded to fp32 on its own on both sides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import META, W_SEED
from super_resolution_amd import synth, y4m, yuv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLED = ("nv12", "i420", "i422", "nv16")
SITED = ("left", "topleft")
DEPTHS = [(8, None), (10, True), (10, False)]
DEPTH_IDS = ["8", "10msb", "10lsb"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _net(arch, name, dtype, dev, **kw):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(type=arch, compute_dtype=dtype, **dict(META["cfgs"][name], **kw))).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    return net.to(dev)


def _sub(fmt):
    return None if yuv.LAYOUTS[fmt][0] is None else yuv.LAYOUTS[fmt][:2]


def _frames(seed, B, h, w, fmt, depth=8, msb=None):
    """Random stored samples; LSB-aligned deep words also go above the code range (they saturate), MSB-aligned ones carry low bits."""
    dt = yuv.container(depth, fmt, msb)[0]
    return np.random.default_rng(seed).integers(0, 256 if depth == 8 else 65536, (B,) + yuv.frame_shape_fmt(h, w, fmt)).astype(dt)


def _t(a, dev):
    return torch.from_numpy(a).to(dev) if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)


def _n(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _spaced(a, dev, fill=99):
    """The frames a (B, rows, w) on the device with a batch stride three rows larger than a frame (rows stay packed)."""
    B, rows, w = a.shape
    big = torch.full((B, rows + 3, w), fill, dtype=torch.uint8 if a.dtype == np.uint8 else torch.int16, device=dev)
    big = big if a.dtype == np.uint8 else big.view(torch.uint16)
    view = big[:, 1:1 + rows]
    _raw(view).copy_(_raw(_t(a, dev)))
    assert view.stride(0) == (rows + 3) * w and view.stride(1) == w
    return big, view


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("siting", SITED)
@pytest.mark.parametrize("fmt", SUBSAMPLED)
def test_yuv_to_planes_sited_is_the_definition(fmt, siting, dm):
    """(6, 262) padded to (8, 264): two 256-thread blocks a row, reflected rows and columns, the clamped last chroma column and row;
    and (2, 2), where every neighbour is the sample itself.  B = 2 with samples more than a frame apart."""
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    in_msb = bool(yuv.container(depth, fmt, msb)[3])
    to_rgb = yuv.csc("bt709", False, depth)[0]
    for (h, w), (Hp, Wp) in (((6, 262), (8, 264)), ((6, 262), (6, 262)), ((2, 2), (3, 3)), ((2, 2), (2, 2))):
        frame = _frames(h + w + Hp, 2, h, w, fmt, depth, msb)
        _, d = _spaced(frame, dev)
        big = torch.full((2 * 3 * Hp * Wp + 64,), -7.0, device=dev)
        dst = big[32:-32].view(2, 3, Hp, Wp)
        ops.yuv_to_planes(*ops.yuv_views(d, fmt), dst, to_rgb, sub=_sub(fmt), depth=depth, msb=in_msb, siting=siting)
        torch.cuda.synchronize()
        ref = yuv.yuv_to_planes(frame, fmt=fmt, matrix="bt709", pad=(Hp - h, Wp - w), depth=depth, msb=msb, siting=siting)
        assert np.array_equal(dst.cpu().numpy(), ref), (h, w, Hp, Wp)
        assert bool((big[:32] == -7.0).all()) and bool((big[-32:] == -7.0).all()), "floats outside the planes are not the kernel's"


# ---------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def planes():
    """(2, 3, 10, 1034) in [-0.1, 1.1]: values on both sides of the clamps, wider than one block of 256 four-column threads."""
    rng = np.random.default_rng(16)
    return (rng.random((2, 3, 10, 1034), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)


def _empty(B, h, w, fmt, depth, dev, fill=99):
    dt = torch.uint8 if depth == 8 else torch.int16
    t = torch.full((B,) + yuv.frame_shape_fmt(h, w, fmt), fill, dtype=dt, device=dev)
    return t if depth == 8 else t.view(torch.uint16)


@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("siting", SITED)
@pytest.mark.parametrize("fmt", SUBSAMPLED)
def test_planes_to_yuv_sited_is_the_definition(fmt, siting, dm, planes):
    """Crops (6, 1030) and (10, 1034): the block boundary at column 1024 (its first thread takes column 1023 from the block before),
    the n = 2 tail, a crop narrower and lower than the planes, the first row's and column's clamps; and (2, 2)."""
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    src = torch.from_numpy(planes).to(dev)
    out_msb = bool(yuv.container(depth, fmt, msb)[3])
    from_rgb = yuv.csc("bt601", True, depth)[1]
    for crop in ((6, 1030), (10, 1034), (2, 2)):
        ref = yuv.planes_to_yuv(planes, fmt=fmt, matrix="bt601", full_range=True, crop=crop, out_depth=depth, msb=msb, siting=siting)
        out = _empty(2, *crop, fmt, depth, dev)
        ops.planes_to_yuv(src, *ops.yuv_views(out, fmt), from_rgb, sub=_sub(fmt), depth=depth, msb=out_msb, siting=siting)
        torch.cuda.synchronize()
        assert np.array_equal(_n(out), ref), crop
        centre = yuv.planes_to_yuv(planes, fmt=fmt, matrix="bt601", full_range=True, crop=crop, out_depth=depth, msb=msb)
        assert not np.array_equal(ref, centre), "(the case tells the sitings apart)"


@pytest.mark.parametrize("fmt", ["nv12", "i422", "i444", "gray"])
def test_siting_zero_and_ignored_sitings_through_the_sited_entries_are_the_unsited_entries(fmt, planes):
    """Code 0 — and every code on a surface without a subsampled axis — forwards to the unsited entry: the same samples, both ways."""
    dev = _dev()
    from super_resolution_amd import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    sub = _sub(fmt)
    codes = (0,) if sub is not None and sub[0] == 1 else (0, 1, 2)
    to_rgb, from_rgb = ops._f12(yuv.csc()[0]), ops._f12(yuv.csc()[1])
    h, w = 6, 262
    d = _t(_frames(3, 2, h, w, fmt), dev)
    views = ops.yuv_views(d, fmt)
    surf = ops.yuv_surface(*views, sub=sub)
    want = torch.empty(2, 3, 8, 264, device=dev)
    ops.yuv_to_planes(*views, want, yuv.csc()[0], sub=sub)
    src = torch.from_numpy(planes).to(dev)
    want_out = _empty(2, 6, 1030, fmt, 8, dev)
    ops.planes_to_yuv(src, *ops.yuv_views(want_out, fmt), yuv.csc()[1], sub=sub)
    for code in codes:
        got = torch.full_like(want, -1.0)
        _lib.check(lib.hat_yuv_to_planes_sited(C.byref(surf), code, got.data_ptr(), 2, h, w, 8, 264, to_rgb, st), "hat_yuv_to_planes_sited")
        out = _empty(2, 6, 1030, fmt, 8, dev, 55)
        ov = ops.yuv_views(out, fmt)
        osurf = ops.yuv_surface(*ov, sub=sub)
        _lib.check(lib.hat_planes_to_yuv_sited(src.data_ptr(), 2, 10, 1034, C.byref(osurf), code, 6, 1030, from_rgb, st), "hat_planes_to_yuv_sited")
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(out, want_out), code
        if code:
            assert np.array_equal(_n(out), yuv.planes_to_yuv(planes, fmt=fmt, crop=(6, 1030), siting=yuv.SITINGS[code]))


# ---------------------------------------------------------------------------------------------- 3
# arch, model, (B, h, w), fmt, out_fmt, siting, out_siting, ensemble; 13 x 22, 17 x 31 and 12 x 14 need reflection padding
CASES = [("HAT", "hats_1g_x4", (1, 32, 48), "nv12", "nv12", "left", None, 1),
         ("HATX", "hatx_tiny_plain_x2", (2, 13, 22), "i422", "i444", "left", None, 1),
         ("HAT", "hats_1g_x4", (1, 17, 31), "i444", "nv12", "center", "topleft", 1),
         ("HATX", "hatx_tiny_plain_x2", (1, 12, 14), "i420", "i420", "topleft", None, 2)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[1]}_{c[3]}_{c[5]}_to_{c[4]}_{c[6]}_B{c[2][0]}_e{c[7]}" for c in CASES])
def test_forward_yuv_sited_is_the_composition(case, dtype):
    dev = _dev()
    arch, name, (B, h, w), fmt, out_fmt, siting, out_siting, ens = case
    cfg = META["cfgs"][name]
    ws, s = cfg["window_size"], cfg["upscale"]
    net = _net(arch, name, dtype, dev)
    eng = net.engine(dev)
    frames = _frames(h * w + B, B, h, w, fmt)
    pad = ((ws - h % ws) % ws, (ws - w % ws) % ws)
    x = torch.from_numpy(yuv.yuv_to_planes(frames, fmt=fmt, matrix="bt709", pad=pad, siting=siting)).to(dev)
    y = (net(x) if ens == 1 else net.forward_ensemble(x, ens)).cpu().numpy()
    osit = siting if out_siting is None else out_siting
    ref = yuv.planes_to_yuv(y, fmt=out_fmt, matrix="bt709", crop=(s * h, s * w), siting=osit)
    kw = dict(fmt=fmt, out_fmt=out_fmt, matrix="bt709", ensemble=ens, siting=siting, out_siting=out_siting)
    before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
    out = net.forward_yuv(_t(frames, dev), **kw)
    assert tuple(out.shape) == (B,) + yuv.frame_shape_fmt(s * h, s * w, out_fmt)
    assert np.array_equal(_n(out), ref)
    if yuv.effective_siting(_sub(out_fmt), osit) != "center":
        assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (before[0], before[1] + 1), "a sited output ends in planes"
    mine = _empty(B, s * h, s * w, out_fmt, 8, dev, 0)
    assert net.forward_yuv(_t(frames, dev), out=mine, **kw) is mine and np.array_equal(_n(mine), ref), "out= is filled with the same samples"
    if fmt == out_fmt and fmt in yuv.FORMATS:
        kw420 = dict(fmt=fmt, matrix="bt709", ensemble=ens, siting=siting, out_siting=out_siting)
        assert np.array_equal(_n(net.forward_yuv420(_t(frames, dev), **kw420)), ref), "forward_yuv420 takes the same arguments"


def test_counters_and_the_fused_epilogue():
    """tiny_x3 (window 8, x3) at 16 columns: conv_last's row sweep has its epilogue (wd = 48).  A centre output fuses as today,
    whatever the INPUT siting; an output with a co-sited axis ends in hat_conv3x3_to_planes + hat_planes_to_yuv_sited."""
    dev = _dev()
    net = _net("HAT", "tiny_x3", "bf16", dev)
    eng = net.engine(dev)
    frames = _frames(16, 1, 8, 16, "i420")
    for siting, out_siting, out_fmt, fused in (("center", "center", "i420", True), ("left", "center", "i420", True), ("left", None, "i420", False),
                                               ("center", "topleft", "nv16", False), ("left", "left", "i444", True), ("topleft", None, "gray", True)):
        before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
        out = net.forward_yuv(_t(frames, dev), fmt="i420", out_fmt=out_fmt, siting=siting, out_siting=out_siting)
        assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (before[0] + int(fused), before[1] + int(not fused)), (siting, out_siting, out_fmt)
        y = net(torch.from_numpy(yuv.yuv_to_planes(frames, fmt="i420", siting=siting)).to(dev)).cpu().numpy()
        assert np.array_equal(_n(out), yuv.planes_to_yuv(y, fmt=out_fmt, siting=siting if out_siting is None else out_siting))
    with pytest.raises(RuntimeError, match="SITINGS"):
        net.forward_yuv(_t(frames, dev), fmt="i420", siting="mpeg2")
    with pytest.raises(RuntimeError, match="SITINGS"):
        net.forward_yuv420(_t(frames, dev), out_siting="bottom")


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("W", [16, 8], ids=["ends_in_conv3x3_to_planes", "ends_in_conv"])
def test_plan_forward_yuv_sited(W, tmp_path):
    """tiny_x3 recorded at width 16 ends in hat_conv3x3_to_planes (a centre output replays it as the fused epilogue, a sited one
    into the staging image), at width 8 it does not; either way the plan writes what HAT.forward_yuv writes."""
    dev = _dev()
    from super_resolution_amd import plan
    net = _net("HAT", "tiny_x3", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 8, W), path)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    for (h, w), fmt, out_fmt, siting, out_siting in (((8, W), "i420", "i420", "left", None), ((6, W - 2), "nv12", "nv12", "topleft", None),
                                                     ((8, W), "i422", "i420", "left", "topleft"), ((8, W), "i420", "i422", "left", "center"),
                                                     ((8, W), "i420", "i420", "center", "left"), ((8, W), "i444", "gray", "topleft", None)):
        frames = _t(_frames(h + w, 1, h, w, fmt), dev)
        kw = dict(fmt=fmt, out_fmt=out_fmt, matrix="bt709", siting=siting, out_siting=out_siting)
        ref = net.forward_yuv(frames, **kw)
        out = _empty(1, 3 * h, 3 * w, out_fmt, 8, dev, 9)
        p.forward_yuv(frames, out, stream=stream, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (h, w, fmt, out_fmt, siting, out_siting)
    frames = _t(_frames(5, 1, 8, W, "nv12"), dev)
    out = _empty(1, 24, 3 * W, "nv12", 8, dev, 9)
    p.forward_yuv420(frames, out, fmt="nv12", siting="left", stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(out, net.forward_yuv420(frames, fmt="nv12", siting="left"))
    p.close()


# ---------------------------------------------------------------------------------------------- 5, 6
@pytest.fixture(scope="module")
def mpeg2_file(tmp_path_factory):
    """Two 28 x 44 frames in a C420mpeg2 file (they pad to 32 x 48)."""
    d = tmp_path_factory.mktemp("siting")
    h, w = 28, 44
    seq = [_frames(400 + i, 1, h, w, "i420")[0] for i in range(2)]
    hdr = {"W": w, "H": h, "F": "25:1", "I": "p", "A": "1:1", "C": "420mpeg2", "X": []}
    with y4m.Writer(str(d / "in.y4m"), hdr) as wr:
        for f in seq:
            wr.write(f)
    return str(d / "in.y4m"), hdr, seq


def test_c_example_with_chroma_loc_left(mpeg2_file, tmp_path):
    dev = _dev()
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs the HIP headers")
    from super_resolution_amd import frames as FR, plan
    src, hdr, seq = mpeg2_file
    exe = tmp_path / "plan_upscale_y4m_chroma"
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_y4m_chroma.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    net = _net("HAT", "hats_1g_x4", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 32, 48), path)
    want = list(FR.upscale_frames(net, iter(seq), pixfmt="i420", siting="left"))
    centre = list(FR.upscale_frames(net, iter(seq), pixfmt="i420"))
    assert not np.array_equal(want[0], centre[0])
    for args, ref in ((["--chroma-loc", "left"], want), ([], centre)):
        r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, src, str(tmp_path / "out.y4m")] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        with y4m.Reader(str(tmp_path / "out.y4m")) as rd:
            assert rd.header == y4m.scaled_header(hdr, 4)
            got = list(rd)
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, ref)), args


def test_video_tool_auto_is_left_for_a_mpeg2_file(mpeg2_file, tmp_path):
    dev = _dev()
    from super_resolution_amd import video
    src, hdr, seq = mpeg2_file
    net = _net("HATX", "hatx_tiny_plain_x2", "bf16", dev)
    base = ["-opt", "o.yml", "-i", src, "-o", "b"]
    outs = {}
    for name, extra in (("auto", ["--chroma-loc", "auto"]), ("left", ["--chroma-loc", "left"]), ("default", [])):
        a = video.parser().parse_args(base + extra)
        info = video.upscale_file(net, a.input, str(tmp_path / f"{name}.y4m"), chroma_loc=a.chroma_loc, out_chroma_loc=a.out_chroma_loc)
        assert info["frames"] == 2 and info.get("chroma_loc") == (None if name == "default" else "left")
        with y4m.Reader(str(tmp_path / f"{name}.y4m")) as rd:
            assert rd.header == y4m.scaled_header(hdr, 2) and rd.header["C"] == "420mpeg2"
            outs[name] = list(rd)
    want = [net.forward_yuv420(torch.from_numpy(f).to(dev), fmt="i420", siting="left")[0].cpu().numpy() for f in seq]
    assert all(np.array_equal(a, b) for a, b in zip(outs["auto"], outs["left"]))
    assert all(np.array_equal(a, b) for a, b in zip(outs["left"], want))
    today = [net.forward_yuv420(torch.from_numpy(f).to(dev), fmt="i420")[0].cpu().numpy() for f in seq]
    assert all(np.array_equal(a, b) for a, b in zip(outs["default"], today)), "the default treats the file as before"
    assert not np.array_equal(outs["default"][0], outs["left"][0])
