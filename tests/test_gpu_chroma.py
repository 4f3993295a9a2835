"""4:2:2, 4:4:4 and grey on the GPU, any subsampling in and out: the surface kernels, the fused epilogue, forward_yuv, the plans, the C
example, the frame generator and the file tool.  Every comparison with the definition (super_resolution_amd/yuv.py, pinned to the
reference by tests/test_chroma_cpu.py) is an equality: every product and sum of the conversion is rounded to fp32 on its own on
both sides."""
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import META, W_SEED
from super_resolution_amd import synth, y4m, yuv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("i422", "nv16", "i444", "nv24", "gray")
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
    """numpy frames -> device tensor (uint16 goes through int16: the same words)."""
    return torch.from_numpy(a).to(dev) if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)


def _n(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _empty(B, h, w, fmt, depth, dev, fill=99):
    dt = torch.uint8 if depth == 8 else torch.int16
    t = torch.full((B,) + yuv.frame_shape_fmt(h, w, fmt), fill, dtype=dt, device=dev)
    return t if depth == 8 else t.view(torch.uint16)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("fmt", NEW)
def test_yuv_to_planes_is_the_definition(fmt, dm):
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    B, h, w = 2, 29, (262 if yuv.LAYOUTS[fmt][0] == 1 else 261)      # straddles the 256-thread row segment; odd where allowed
    frame = _frames(h + w, B, h, w, fmt, depth, msb)
    d = _t(frame, dev)
    views = ops.yuv_views(d, fmt)
    in_msb = bool(yuv.container(depth, fmt, msb)[3])
    to_rgb = yuv.csc("bt709", False, depth)[0]
    for pad in ((0, 0), (6, 0), (0, 6), (6, 6)):
        Hp, Wp = h + pad[0], w + pad[1]
        big = torch.full((B * 3 * Hp * Wp + 64,), -7.0, device=dev)
        dst = big[32:-32].view(B, 3, Hp, Wp)
        ops.yuv_to_planes(*views, dst, to_rgb, sub=_sub(fmt), depth=depth, msb=in_msb)
        torch.cuda.synchronize()
        ref = yuv.yuv_to_planes(frame, fmt=fmt, matrix="bt709", pad=pad, depth=depth, msb=msb)
        assert np.array_equal(dst.cpu().numpy(), ref), pad
        assert bool((big[:32] == -7.0).all()) and bool((big[-32:] == -7.0).all()), "floats outside the planes are not the kernel's"


# ---------------------------------------------------------------------------------------------- 2
def _special_planes(B, Hs, Ws):
    """tests/test_gpu_yuv.py's special values: zeros of both signs, 1 and its successor, the infinities, every k / 255, every
    half-way point between two 8-bit levels with its fp32 neighbours, and uniform values in [-0.5, 1.5)."""
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
    for c in range(3):
        t[0, c, 100 * c:100 * c + sp.numel()] = sp
    return t.reshape(B, 3, Hs, Ws)


@pytest.fixture(scope="module")
def special():
    return _special_planes(2, 31, 61)


@pytest.mark.parametrize("dm", DEPTHS[:2], ids=DEPTH_IDS[:2])
@pytest.mark.parametrize("fmt", NEW)
def test_planes_to_yuv_is_the_definition(fmt, dm, special):
    """Crops whose widths leave tails of 1, 2 and 3 columns behind the four-column threads (2 at 4:2:2, whose widths are even);
    once into the packed layout (the vector stores) and once into views that start at an odd byte offset with odd pitches (8-bit:
    single-sample stores)."""
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    B, sx = 2, yuv.LAYOUTS[fmt][0]
    src = special.to(dev)
    out_msb = bool(yuv.container(depth, fmt, msb)[3])
    from_rgb = yuv.csc("bt601", True, depth)[1]
    for crop in ([(31, 58), (30, 60)] if sx == 1 else [(31, 61), (30, 58), (29, 59), (31, 60)]):
        ho, wo = crop
        ref = yuv.planes_to_yuv(special.numpy(), fmt=fmt, matrix="bt601", full_range=True, crop=crop, out_depth=depth, msb=msb)
        packed = _empty(B, ho, wo, fmt, depth, dev)
        ops.planes_to_yuv(src, *ops.yuv_views(packed, fmt), from_rgb, sub=_sub(fmt), depth=depth, msb=out_msb)
        torch.cuda.synchronize()
        assert np.array_equal(_n(packed), ref), crop
        if depth != 8:
            continue
        # the same samples behind pitched views from an odd address: Y rows wo + 3 apart, chroma rows their length + 1 apart
        sub = _sub(fmt)
        ybuf = torch.full((B * ho * (wo + 3) + 1,), 99, dtype=torch.uint8, device=dev)
        y = ybuf[1:].view(B, ho, wo + 3)[:, :, :wo]
        assert y.data_ptr() % 2 == 1
        cb = cr = cbuf = None
        if sub is not None:
            ch, cw = ho >> sub[1], wo >> sub[0]
            step = 1 if yuv.LAYOUTS[fmt][2] == "planar" else 2
            cbuf = torch.full((2 if step == 1 else 1, B * ch * (step * cw + 1) + 1), 99, dtype=torch.uint8, device=dev)
            rows = lambda k: cbuf[k, 1:].view(B, ch, step * cw + 1)
            cb, cr = (rows(0)[:, :, :cw], rows(1)[:, :, :cw]) if step == 1 else (rows(0)[:, :, 0:2 * cw:2], rows(0)[:, :, 1:2 * cw:2])
        ops.planes_to_yuv(src, y, cb, cr, from_rgb, sub=sub, depth=8)
        torch.cuda.synchronize()
        ry, rcb, rcr = yuv.split_fmt(ref, fmt)
        assert np.array_equal(y.cpu().numpy(), ry), crop
        assert bool((ybuf[1:].view(B, ho, wo + 3)[:, :, wo:] == 99).all()) and int(ybuf[0]) == 99, "bytes between the rows are not the kernel's"
        if sub is not None:
            assert np.array_equal(cb.cpu().numpy(), rcb) and np.array_equal(cr.cpu().numpy(), rcr), crop
            assert bool((cbuf[:, 0] == 99).all()) and bool((cbuf[:, 1:].reshape(cbuf.shape[0], B, ch, -1)[..., -1] == 99).all())


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("shape", [(24, 16), (24, 48), (72, 5120)], ids=["24x16", "24x48", "72x5120"])
def test_conv3x3_to_yuv_equals_planes_then_convert(shape):
    """test_conv3x3_to_yuv420_equals_planes_then_convert's shapes (strips, bands, several trips) for every output subsampling, 8 and
    10 bits, with crops that are odd where the subsampling allows it."""
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
    for fmt in ("i420", "nv12") + NEW:
        sx, sy, _ = yuv.LAYOUTS[fmt]
        crops = [(H, W), (H - 3 + (sy == 1), W - 5 + (sx == 1)), (1 + (sy == 1), 1 + (sx == 1))]
        for depth in (8, 10):
            msb = bool(yuv.container(depth, fmt)[3])
            m = yuv.csc("bt709", True, depth)[1]
            for ho, wo in crops:
                ref, out = _empty(B, ho, wo, fmt, depth, dev, 77), _empty(B, ho, wo, fmt, depth, dev, 55)
                ops.planes_to_yuv(planes, *ops.yuv_views(ref, fmt), m, sub=_sub(fmt), depth=depth, msb=msb)
                ops.conv3x3_to_yuv(x, wpk, b8, *ops.yuv_views(out, fmt), sub=_sub(fmt), from_rgb=m, depth=depth, msb=msb, **kw)
                torch.cuda.synchronize()
                assert np.array_equal(_n(out), _n(ref)), (fmt, depth, ho, wo)


# ---------------------------------------------------------------------------------------------- 4
# arch, model, (B, h, w), fmt, out_fmt, depth, out_depth, ensemble; 13 x 22 and 17 x 31 need reflection padding
CASES = [("HAT", "hats_1g_x4", (1, 32, 48), "nv12", "i444", 8, 8, 1),
         ("HATX", "hatx_tiny_plain_x2", (2, 13, 22), "i422", "i422", 8, 8, 1),
         ("HAT", "hats_1g_x4", (1, 17, 31), "i444", "nv12", 8, 8, 1),
         ("HATX", "hatx_tiny_plain_x2", (1, 11, 13), "gray", "gray", 8, 8, 2),
         ("HATX", "hatx_tiny_plain_x2", (1, 16, 24), "nv16", "nv24", 10, 10, 1),
         ("HAT", "hats_1g_x4", (1, 32, 32), "i420", "i444", 8, 10, 1)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[1]}_{c[3]}{c[5]}_to_{c[4]}{c[6]}_B{c[2][0]}_e{c[7]}" for c in CASES])
def test_forward_yuv_is_the_composition(case, dtype):
    dev = _dev()
    arch, name, (B, h, w), fmt, out_fmt, depth, out_depth, ens = case
    cfg = META["cfgs"][name]
    ws, s = cfg["window_size"], cfg["upscale"]
    net = _net(arch, name, dtype, dev)
    frames = _frames(h * w + B, B, h, w, fmt, depth)
    pad = ((ws - h % ws) % ws, (ws - w % ws) % ws)
    x = torch.from_numpy(yuv.yuv_to_planes(frames, fmt=fmt, matrix="bt709", pad=pad, depth=depth)).to(dev)
    y = (net(x) if ens == 1 else net.forward_ensemble(x, ens)).cpu().numpy()
    ref = yuv.planes_to_yuv(y, fmt=out_fmt, matrix="bt709", crop=(s * h, s * w), out_depth=out_depth)
    kw = dict(fmt=fmt, matrix="bt709", depth=depth, ensemble=ens)
    if out_fmt != fmt:
        kw["out_fmt"] = out_fmt
    if out_depth != depth:
        kw["out_depth"] = out_depth
    out = net.forward_yuv(_t(frames, dev), **kw)
    assert tuple(out.shape) == (B,) + yuv.frame_shape_fmt(s * h, s * w, out_fmt) and out.dtype == (torch.uint8 if out_depth == 8 else torch.uint16)
    assert np.array_equal(_n(out), ref)
    mine = _empty(B, s * h, s * w, out_fmt, out_depth, dev, 0)
    assert net.forward_yuv(_t(frames, dev), out=mine, **kw) is mine and np.array_equal(_n(mine), ref), "out= is filled with the same samples"
    if B == 1:
        assert np.array_equal(_n(net.forward_yuv(_t(frames, dev)[0], **kw)), ref), "(rows, w) is accepted as one frame"


@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_forward_yuv_is_forward_yuv420_for_the_old_formats(fmt):
    dev = _dev()
    net = _net("HATX", "hatx_tiny_plain_x2", "bf16", dev)
    for depth, (h, w) in ((8, (14, 20)), (10, (16, 24))):
        d = _t(_frames(7, 2, h, w, fmt, depth), dev)
        assert torch.equal(_raw(net.forward_yuv(d, fmt=fmt, depth=depth)), _raw(net.forward_yuv420(d, fmt=fmt, depth=depth)))


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


@pytest.mark.parametrize("out_fmt", yuv.ALL_FORMATS)
def test_the_two_counters_follow_todays_rule_for_every_output_format(out_fmt):
    """tiny_x3 (window 8, x3): a 16-column frame gives wd = 48 (the fused epilogue), an 8-column one wd = 24 (planes, then
    hat_planes_to_yuv); the samples are the definition's either way."""
    dev = _dev()
    net = _net("HAT", "tiny_x3", "bf16", dev)
    eng = net.engine()
    for w, fused in ((16, True), (8, False)):
        frames = _frames(w, 1, 8, w, "i420")
        before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
        out = net.forward_yuv(_t(frames, dev), fmt="i420", out_fmt=out_fmt)
        assert (eng.yuv_fused_calls, eng.yuv_planes_calls) == (before[0] + int(fused), before[1] + int(not fused)), (w, out_fmt)
        y = net(torch.from_numpy(yuv.yuv_to_planes(frames, fmt="i420")).to(dev)).cpu().numpy()
        assert np.array_equal(_n(out), yuv.planes_to_yuv(y, fmt=out_fmt))


def test_forward_yuv_refusals():
    dev = _dev()
    net = _net("HAT", "tiny_x3", "f32", dev)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="even width"):
        net.forward_yuv(z(1, 32, 15), fmt="i422")
    with pytest.raises(RuntimeError, match="even height"):
        net.forward_yuv(z(1, 45, 16), fmt="i444", out_fmt="i420")     # 15 x 16 in, 45 x 48 out: no 4:2:0 frame
    with pytest.raises(RuntimeError, match="format"):
        net.forward_yuv(z(1, 32, 16), fmt="i444", out_fmt="yuyv")
    with pytest.raises(RuntimeError, match="reflect"):
        net.forward_yuv(z(1, 4, 16), fmt="gray")
    with pytest.raises(TypeError, match="uint16"):
        net.forward_yuv(z(1, 16, 16), fmt="gray", depth=10)
    with pytest.raises(RuntimeError, match="out must be"):
        net.forward_yuv(z(1, 16, 16), fmt="gray", out_fmt="i444", out=z(1, 48, 48))


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", [("HAT", "hats_1g_x4", "bf16", (1, 3, 32, 48), (28, 42), "nv12", "i444", 8, 10),
                                  ("HATX", "hatx_tiny_plain_x2", "f32", (2, 3, 16, 24), (13, 20), "i422", "gray", 10, 8)],
                         ids=["hats_bf16_nv12_to_i444p10", "hatx_f32_B2_i422p10_to_gray"])
def test_plan_forward_yuv(case, tmp_path):
    dev = _dev()
    from super_resolution_amd import plan
    arch, name, dtype, shape, small, fmt, out_fmt, depth, out_depth = case
    B, _, H, W = shape
    s = META["cfgs"][name]["upscale"]
    net = _net(arch, name, dtype, dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, shape, path)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(fmt=fmt, out_fmt=out_fmt, matrix="bt709", full_range=True, depth=depth, out_depth=out_depth)
    for h, w in ((H, W), small):                                 # the smaller frame pads to the plan's shape, as forward_yuv pads it
        frames = _t(_frames(h + w, B, h, w, fmt, depth), dev)
        ref = net.forward_yuv(frames, **kw)
        out = _empty(B, s * h, s * w, out_fmt, out_depth, dev, 9)
        p.forward_yuv(frames, out, stream=stream, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_raw(out), _raw(ref)), (h, w)
    p.close()


# ---------------------------------------------------------------------------------------------- 6
def test_c_example_on_a_422p10_file(tmp_path):
    dev = _dev()
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs the HIP headers")
    from super_resolution_amd import plan
    exe = tmp_path / "plan_upscale_y4m_chroma"
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_y4m_chroma.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    net = _net("HAT", "hats_1g_x4", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 32, 48), path)
    h, w = 27, 44
    frames = [_frames(80 + i, 1, h, w, "i422", 10, False)[0] & 1023 for i in range(2)]
    hdr = {"W": w, "H": h, "F": "25:1", "I": "p", "A": "1:1", "C": "422p10", "X": []}
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr, chroma=True) as wr:
        for f in frames:
            wr.write(f)
    for args, out_fmt, out_depth, c in (([], "i422", 10, "422p10"), (["444", "8"], "i444", 8, "444")):
        want = [_n(net.forward_yuv(_t(f, dev), fmt="i422", out_fmt=out_fmt, depth=10, out_depth=out_depth))[0] for f in frames]
        r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")] + args,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        with y4m.Reader(str(tmp_path / "out.y4m"), chroma=True) as rd:
            assert rd.header == dict(y4m.scaled_header(hdr, 4), C=c) and rd.fmt == out_fmt
            got = list(rd)
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------- 7
def test_upscale_frames_422_to_444_matches_forward_yuv_in_order():
    dev = _dev()
    from super_resolution_amd import frames as FR
    net = _net("HATX", "hatx_tiny_plain_x2", "bf16", dev)
    h, w = 13, 22
    seq = [_frames(200 + i, 1, h, w, "i422")[0] for i in range(4)]
    want = [net.forward_yuv(torch.from_numpy(f).to(dev), fmt="i422", out_fmt="i444")[0].cpu().numpy() for f in seq]
    got = list(FR.upscale_frames(net, iter(seq), pixfmt="i422", out_pixfmt="i444"))
    assert len(got) == 4 and all(a.shape == yuv.frame_shape_fmt(2 * h, 2 * w, "i444") for a in got)
    for i in range(4):
        assert np.array_equal(got[i], want[i]), f"frame {i}"
    with pytest.raises(RuntimeError, match="out_pixfmt"):
        next(FR.upscale_frames(net, iter(seq), pixfmt="i422", out_pixfmt="rgb24"))


@pytest.mark.parametrize("c", ["444", "mono"])
def test_upscale_file_writes_what_the_reader_reads_back(c, tmp_path):
    dev = _dev()
    from super_resolution_amd import video
    net = _net("HATX", "hatx_tiny_plain_x2", "bf16", dev)
    fmt, (h, w) = y4m.CHROMAS[c], (11, 13)
    seq = [_frames(300 + i, 1, h, w, fmt)[0] for i in range(3)]
    hdr = {"W": w, "H": h, "F": "24:1", "C": c, "X": ["COLORRANGE=LIMITED"]}
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr, chroma=True) as wr:
        for f in seq:
            wr.write(f)
    info = video.upscale_file(net, str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), matrix="bt709")
    assert info == {"frames": 3, "in": (w, h), "out": (2 * w, 2 * h), "chroma": c, "out_chroma": c}
    with y4m.Reader(str(tmp_path / "out.y4m"), chroma=True) as rd:
        assert rd.header == y4m.scaled_header(hdr, 2) and rd.fmt == fmt
        got = list(rd)
    want = [net.forward_yuv(torch.from_numpy(f).to(dev), fmt=fmt, matrix="bt709")[0].cpu().numpy() for f in seq]
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    if c == "444":                                               # and down to 4:2:0 on the way out
        info = video.upscale_file(net, str(tmp_path / "in.y4m"), str(tmp_path / "out420.y4m"), out_chroma="420")
        with y4m.Reader(str(tmp_path / "out420.y4m")) as rd:    # a plain 4:2:0 stream: no keyword needed
            assert rd.header["C"] == "420" and info["out_chroma"] == "420"
            assert np.array_equal(next(rd), net.forward_yuv(torch.from_numpy(seq[0]).to(dev), fmt="i444", out_fmt="i420")[0].cpu().numpy())
