"""ESC-LTE's frame paths on the device.  Kernel level: the byte and YCbCr sinks of hat_lte_query's grid mode (ops.lte_query_u8,
ops.lte_query_yuv) against the two-step route — ops.lte_query's grid planes, then ops.planes_to_u8 / ops.planes_to_yuv — BIT FOR
BIT: the fp32 image value and the conversion are the same expressions, so a difference is a bug, not a tolerance question.  Whole
model: ESCLTE.upscale_u8 / upscale_yuv against the composition of the calls they fuse, bit for bit; against the host definition
yuv.planes_to_yuv; against the reference's restatement in fp64 (tests/esclte_ref.py, itself held to 1e-5 of the goldens); and
frames.upscale_frames with size=.

The seeded head of tests/esclte_ref.py on the 5 x 7 map gives images (out_affine (0.5, 0.5)) from about -0.35 to 1.18 on every grid
used here (computed on the host in fp64), so both clamps of both conversions are hit; the tests assert it of the device's planes."""
import functools

import numpy as np
import pytest
import torch

import esclte_ref as R
from test_gpu_esclte import DT, _dev, _net, device_head

pytestmark = pytest.mark.gpu

MAP = (5, 7)
EVEN = [(4, 8), (6, 10), (10, 18)]    # one exact tile; ragged in both axes, 2 x 2 tiles; 3 x 3 tiles
ODD = [(5, 7), (11, 13)]
# 12288 pixels at 16 bits: a code step is 1.8e-5 of the image range, so a last-bit difference between the sink's fp32 value and the
# plane store's (two instantiations whose products and sums the compiler fused differently gave one) moves about one code in 300 and
# shows here; on the small grids at 8 bits it would not
BIG = (96, 128)
BT601 = dict(matrix="bt601", full_range=False)
SUB = {"i420": (1, 1), "nv12": (1, 1), "nv21": (1, 1), "i422": (1, 0), "nv16": (1, 0), "i444": (0, 0), "nv24": (0, 0), "gray": None}


def _cell(hw, HW=MAP):
    cy, cx = R.grid_cell(hw, HW, 4)
    return float(cy), float(cx)


def _planes(dtype, hw, HW=MAP):
    """The two-step route's first step: ops.lte_query's grid planes (1,3,h,w) with the affine (0.5, 0.5)."""
    ops, pl, coef, freq, inp, kw = device_head(dtype, *HW)
    planes = torch.full((1, 3) + hw, float("nan"), device=coef.device)
    ops.lte_query(pl, coef, freq, inp, planes, grid=hw, cell_yx=_cell(hw, HW), out_affine=(0.5, 0.5), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(planes).all()
    if HW == MAP:
        assert float(planes.min()) < 0 and float(planes.max()) > 1, f"the {hw} image does not reach both clamps"
    return planes


def _frame_buffer(hw, fmt, depth):
    from super_resolution_amd import yuv
    dt = torch.uint8 if depth == 8 else torch.uint16
    fill = 0xA5 if depth == 8 else 0x5A5A
    return torch.full((1,) + yuv.frame_shape_fmt(*hw, fmt), fill, dtype=torch.int16 if depth != 8 else dt, device=_dev()).view(dt)


def _eq(a, b):
    raw = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
    return torch.equal(raw(a), raw(b))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", EVEN + ODD, ids=lambda g: f"{g[0]}x{g[1]}")
def test_u8_sink_equals_planes_then_planes_to_u8(hw, dtype):
    """bgr False and True, and a pitched out (a column slice of a wider tensor) whose other bytes stay 0xA5."""
    ops, pl, coef, freq, inp, kw = device_head(dtype, *MAP)
    planes = _planes(dtype, hw)
    h, w = hw
    for bgr in (False, True):
        want = torch.empty((1, h, w, 3), dtype=torch.uint8, device=coef.device)
        ops.planes_to_u8(planes, want, bgr=bgr)
        got = torch.full((1, h, w, 3), 0xA5, dtype=torch.uint8, device=coef.device)
        ops.lte_query_u8(pl, coef, freq, inp, got, grid=hw, cell_yx=_cell(hw), out_affine=(0.5, 0.5), bgr=bgr, **kw)
        wide = torch.full((1, h + 2, w + 5, 3), 0xA5, dtype=torch.uint8, device=coef.device)
        ops.lte_query_u8(pl, coef, freq, inp, wide[:, 1:h + 1, 2:w + 2], grid=hw, cell_yx=_cell(hw), out_affine=(0.5, 0.5), bgr=bgr, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"u8 sink {hw} bgr={bgr} [{dtype}]: {int((got != want).sum())} bytes differ"
        assert torch.equal(wide[:, 1:h + 1, 2:w + 2], want), f"pitched u8 sink {hw} bgr={bgr} [{dtype}]"
        outside = wide.clone()
        outside[:, 1:h + 1, 2:w + 2] = 0xA5
        assert bool((outside == 0xA5).all()), f"pitched u8 sink {hw} [{dtype}] wrote outside its rows"
    assert int(want.min()) == 0 and int(want.max()) == 255


YUV_CASES = [(fmt, hw, 8, None) for fmt in ("i420", "nv12", "nv21") for hw in EVEN] \
    + [(fmt, hw, 8, None) for fmt in ("i422", "nv16") for hw in EVEN + [(5, 6)]] \
    + [(fmt, hw, 8, None) for fmt in ("i444", "nv24", "gray") for hw in EVEN + ODD] \
    + [(fmt, (6, 10), 10, msb) for fmt in ("i420", "nv12") for msb in (True, False)] + [("i444", (11, 13), 16, False)] \
    + [(fmt, BIG, 16, False) for fmt in ("i444", "i420")]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("fmt,hw,depth,msb", YUV_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_yuv_sink_equals_planes_then_planes_to_yuv(fmt, hw, depth, msb, dtype):
    """Every layout, centre-sited; the frame buffers start filled, so a sample the sink leaves out shows."""
    from super_resolution_amd import yuv
    ops, pl, coef, freq, inp, kw = device_head(dtype, *MAP)
    planes = _planes(dtype, hw)
    from_rgb = yuv.csc(depth=depth, **BT601)[1]
    msb = bool(yuv.container(depth, fmt, msb)[3])
    want, got = _frame_buffer(hw, fmt, depth), _frame_buffer(hw, fmt, depth)
    ops.planes_to_yuv(planes, *ops.yuv_views(want, fmt), from_rgb, sub=SUB[fmt], depth=depth, msb=msb)
    ops.lte_query_yuv(pl, coef, freq, inp, *ops.yuv_views(got, fmt), from_rgb, grid=hw, cell_yx=_cell(hw), out_affine=(0.5, 0.5),
                      sub=SUB[fmt], depth=depth, msb=msb, **kw)
    torch.cuda.synchronize()
    assert _eq(got, want), f"{fmt} sink {hw} depth {depth} msb {msb} [{dtype}] differs from planes_to_yuv"


@pytest.mark.parametrize("dtype", DT)
def test_sinks_on_a_one_row_map(dtype):
    """The 1 x 3 map (every shift clamps to the one row): the u8 sink on one tile and i420 on a ragged grid."""
    from super_resolution_amd import yuv
    HW = (1, 3)
    ops, pl, coef, freq, inp, kw = device_head(dtype, *HW)
    hw = (4, 8)
    want, got = (torch.full((1,) + hw + (3,), 0xA5, dtype=torch.uint8, device=coef.device) for _ in range(2))
    ops.planes_to_u8(_planes(dtype, hw, HW), want)
    ops.lte_query_u8(pl, coef, freq, inp, got, grid=hw, cell_yx=_cell(hw, HW), out_affine=(0.5, 0.5), **kw)
    hw = (6, 10)
    from_rgb = yuv.csc(**BT601)[1]
    wy, gy = _frame_buffer(hw, "i420", 8), _frame_buffer(hw, "i420", 8)
    ops.planes_to_yuv(_planes(dtype, hw, HW), *ops.yuv_views(wy, "i420"), from_rgb, sub=(1, 1))
    ops.lte_query_yuv(pl, coef, freq, inp, *ops.yuv_views(gy, "i420"), from_rgb, grid=hw, cell_yx=_cell(hw, HW), out_affine=(0.5, 0.5), sub=(1, 1), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(gy, wy)


# ------------------------------------------------------------------------------------------------
# whole model, golden case a (20 x 24 input)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_a_u8():
    """The golden's input as the nearest uint8 frame (20,24,3), on the host."""
    g = R.load_case("a")[2]
    img = torch.from_numpy(g["x"]).double() * 0.5 + 0.5
    return (img[0].permute(1, 2, 0) * 255).round().clamp(0, 255).to(torch.uint8).contiguous()


@functools.lru_cache(maxsize=None)
def case_a_reference():
    """The reference's output for case a's uint8 frame at (30, 41): esclte_ref.upscale in fp64 on float64(u8) / 255, clamped to
    [0, 1] -> (30,41,3) fp64.  (The golden's own output belongs to the unquantised input; the restatement is held to 1e-5 of it by
    tests/test_esclte_cpu.py, and here both sides start from identical bytes.)"""
    cfg, sd, g, meta = R.load_case("a")
    img = (case_a_u8().double() / 255).permute(2, 0, 1)[None]
    y = R.upscale(R.d64(sd), cfg, img, (30, 41), meta["what"]["scale_max"])
    return y[0].permute(1, 2, 0).clamp(0, 1)


def _yuv_frame(fmt, hw=(20, 24), depth=8, seed=3):
    from super_resolution_amd import yuv
    rng = np.random.default_rng(seed)
    planes = rng.random((1, 3) + hw, dtype=np.float32)
    return torch.from_numpy(yuv.planes_to_yuv(planes, fmt=fmt, out_depth=depth, **BT601)).to(_dev())


@pytest.mark.parametrize("dtype", DT)
def test_upscale_u8_equals_the_composition(dtype):
    from super_resolution_amd import ops
    net, _, _ = _net("a", "fp32" if dtype == "f32" else dtype)
    frame = case_a_u8().to(_dev())
    for bgr in (False, True):
        x = torch.empty(1, 3, 20, 24, device=frame.device)
        ops.u8_to_planes(frame[None], x, bgr=bgr)
        want = torch.empty(1, 30, 41, 3, dtype=torch.uint8, device=frame.device)
        ops.planes_to_u8(net.upscale(x, size=(30, 41)), want, bgr=bgr)
        got = net.upscale_u8(frame, size=(30, 41), bgr=bgr)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 30, 41, 3)
        assert torch.equal(got, want), f"upscale_u8 bgr={bgr} [{dtype}]: {int((got != want).sum())} bytes differ"
    assert tuple(net.upscale_u8(frame[None], scale=1.5).shape) == (1, 30, 36, 3)


def _compose_yuv(net, frame, size, fmt, out_fmt, depth=8, out_depth=8, out_siting="center"):
    """yuv_to_planes -> upscale -> planes_to_yuv on the device -> (the frame, upscale's planes)."""
    from super_resolution_amd import ops, yuv
    H, W = yuv.frame_size_fmt(frame.shape, fmt)
    x = torch.empty(1, 3, H, W, device=frame.device)
    ops.yuv_to_planes(*ops.yuv_views(frame, fmt), x, yuv.csc(depth=depth, **BT601)[0], sub=SUB[fmt], depth=depth,
                      msb=bool(yuv.container(depth, fmt, None)[3]))
    planes = net.upscale(x, size=size).contiguous()
    want = _frame_buffer(size, out_fmt, out_depth)
    ops.planes_to_yuv(planes, *ops.yuv_views(want, out_fmt), yuv.csc(depth=out_depth, **BT601)[1], sub=SUB[out_fmt], depth=out_depth,
                      msb=bool(yuv.container(out_depth, out_fmt, None)[3]), siting=out_siting)
    return want, planes


@pytest.mark.parametrize("dtype", DT)
def test_upscale_yuv_equals_the_composition_and_the_host_definition(dtype):
    from super_resolution_amd import yuv
    net, _, _ = _net("a", "fp32" if dtype == "f32" else dtype)
    frame = _yuv_frame("i420")
    want, planes = _compose_yuv(net, frame, (30, 40), "i420", "i420")
    got = net.upscale_yuv(frame[0], size=(30, 40), fmt="i420")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 45, 40)
    assert torch.equal(got, want), f"upscale_yuv i420 [{dtype}]: {int((got != want).sum())} samples differ"
    host = yuv.planes_to_yuv(planes.cpu().numpy(), fmt="i420", **BT601)
    assert np.array_equal(got.cpu().numpy(), host), "upscale_yuv differs from yuv.planes_to_yuv of upscale's planes"
    # another layout out, an odd size, ten bits
    frame = _yuv_frame("nv12")
    want, _ = _compose_yuv(net, frame, (31, 41), "nv12", "i444")
    assert torch.equal(net.upscale_yuv(frame, size=(31, 41), fmt="nv12", out_fmt="i444"), want)
    want, _ = _compose_yuv(net, frame, (30, 40), "nv12", "nv12", out_depth=10)
    assert _eq(net.upscale_yuv(frame, size=(30, 40), fmt="nv12", out_depth=10), want)
    # a co-sited output: the plane query into the workspace, then the sited conversion
    frame = _yuv_frame("i420")
    want, _ = _compose_yuv(net, frame, (30, 40), "i420", "i420", out_siting="left")
    assert torch.equal(net.upscale_yuv(frame, size=(30, 40), fmt="i420", out_siting="left"), want)
    with pytest.raises(ValueError, match="31x40 is no i420 frame"):
        net.upscale_yuv(frame, size=(31, 40), fmt="i420")


def test_out_tensors_and_no_allocation_on_the_second_call():
    net, _, _ = _net("a", "bf16")
    dev = _dev()
    u8, yv = case_a_u8().to(dev), _yuv_frame("i420")
    out_u8 = torch.empty(1, 30, 41, 3, dtype=torch.uint8, device=dev)
    out_yv = torch.empty(1, 45, 40, dtype=torch.uint8, device=dev)
    first = (net.upscale_u8(u8, size=(30, 41), out=out_u8).clone(), net.upscale_yuv(yv, size=(30, 40), fmt="i420", out=out_yv).clone())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert net.upscale_u8(u8, size=(30, 41), out=out_u8) is out_u8
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before, "upscale_u8 with out= allocated on its second call"
    assert net.upscale_yuv(yv, size=(30, 40), fmt="i420", out=out_yv) is out_yv
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before, "upscale_yuv with out= allocated on its second call"
    assert torch.equal(out_u8, first[0]) and torch.equal(out_yv, first[1])
    assert net.engine(dev).ws_allocations == 1
    with pytest.raises(RuntimeError, match="out must be"):
        net.upscale_u8(u8, size=(30, 41), out=out_u8[:, :29])
    with pytest.raises(RuntimeError, match="out must be"):
        net.upscale_yuv(yv, size=(30, 40), fmt="i420", out=out_u8)


@pytest.mark.parametrize("dtype", DT)
def test_upscale_u8_against_the_reference(dtype):
    """fp32: every byte within 1 of the reference's (the project's fp32 bar of 1e-4 in image units is 0.026 of a byte step: only
    rounding ties can move).  bf16: bytes / 255 against the clamped reference at the project's bf16 bar, >= 40 dB and max-abs <=
    0.08 + 0.5 / 255 (the half step is the byte rounding)."""
    net, _, _ = _net("a", "fp32" if dtype == "f32" else dtype)
    ref = case_a_reference()
    got = net.upscale_u8(case_a_u8().to(_dev()), size=(30, 41))[0].cpu()
    ref_u8 = (ref.float() * 255.0).round().to(torch.uint8)
    diff = (got.int() - ref_u8.int()).abs()
    err, db = float((got.double() / 255 - ref).abs().max()), R.psnr(got.double() / 255, ref)
    print(f"upscale_u8 vs the fp64 reference [{dtype}]: {int((diff != 0).sum())} of {diff.numel()} bytes differ, max {int(diff.max())}; "
          f"max-abs {err:.3e}, {db:.1f} dB")
    if dtype == "f32":
        assert int(diff.max()) <= 1
    else:
        assert db >= 40.0 and err <= 0.08 + 0.5 / 255


def test_upscale_frames_with_a_size():
    from super_resolution_amd import frames
    net, _, _ = _net("a", "bf16")
    fs = [_yuv_frame("i420", seed=s)[0] for s in (11, 12, 13)]
    got = list(frames.upscale_frames(net, [f.cpu().numpy() for f in fs], pixfmt="i420", size=(30, 40)))
    assert len(got) == 3 and all(g.shape == (45, 40) and g.dtype == np.uint8 for g in got)
    for g, f in zip(got, fs):
        assert np.array_equal(g, net.upscale_yuv(f, size=(30, 40), fmt="i420")[0].cpu().numpy())
    rgb = [case_a_u8().numpy(), case_a_u8().flip(0).contiguous().numpy()]
    got = list(frames.upscale_frames(net, rgb, scale=1.5))
    assert len(got) == 2 and got[0].shape == (30, 36, 3)
    for g, f in zip(got, rgb):
        assert np.array_equal(g, net.upscale_u8(torch.from_numpy(f).to(_dev()), scale=1.5)[0].cpu().numpy())
