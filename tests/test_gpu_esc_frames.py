"""The ESC family's frame paths on the device.  Kernel level: ops.shuffle_to_u8 / shuffle_to_yuv (hat_shuffle_to_u8 / hat_shuffle_to_yuv)
against the two-step route — ops.esc_shuffle_add (or shuffle_planes), then ops.planes_to_u8 / planes_to_yuv — BIT FOR BIT: the pixel
value is the same one rounded add and the conversion the same device functions, so a difference is a bug, not a tolerance question.
Whole model: upscale_u8 / upscale_yuv / upscale_ensemble of ESC, ESCReal, ESCRealM and ESCFP against the composition over this build's
`forward`, bit for bit on every route (tests/test_gpu_u8.py and test_gpu_yuv.py hold conv_last's fused epilogues to their planes
routes exactly, "exact by construction", and so is the conv route here); the counters name the route; one fp32 check against the CPU
restatement; out=, refusals, and the two command lines."""
import functools

import numpy as np
import pytest
import torch

import ensemble_ref as E
import esc_ref
import escfp_ref
import escreal_ref
import escrealm_ref
from test_gpu_esc import _dev, _net as _esc_net
from test_gpu_escfp import _net as _escfp_net
from test_gpu_escreal import _net as _escreal_net
from test_gpu_escrealm import _net as _escrealm_net

pytestmark = pytest.mark.gpu

BT601 = dict(matrix="bt601", full_range=False)
SUB = {"i420": (1, 1), "nv12": (1, 1), "nv21": (1, 1), "i422": (1, 0), "nv16": (1, 0), "i444": (0, 0), "nv24": (0, 0), "gray": None}
LR, B = (5, 7), 2   # s = 3: 21 columns, five threads of four and a tail of one
DT = ["fp32", "bf16"]


def _eq(a, b):
    raw = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
    return torch.equal(raw(a), raw(b))


@functools.lru_cache(maxsize=None)
def _source(s, ld, with_base):
    """rows (B, H W, ld) and the base image, values from -0.3 to 1.3 so that both clamps of both conversions are hit; the two-step
    route's planes (B,3,sH,sW), computed once per case and left unchanged."""
    from super_resolution_amd import ops
    dev, (H, W) = _dev(), LR
    g = torch.Generator().manual_seed(100 * s + ld + int(with_base))
    rows = (torch.rand(B, H * W, ld, generator=g) * 1.6 - 0.3).to(dev)
    base = ((torch.rand(B, 3, H, W, generator=g) - 0.5) * 0.2).to(dev) if with_base else None
    planes = torch.full((B, 3, s * H, s * W), float("nan"), device=dev)
    if with_base:
        ops.esc_shuffle_add(rows, base, planes, B=B, H=H, W=W, s=s, ld=ld)
    else:
        ops.shuffle_planes(rows, planes, B=B, H=H, W=W, s=s, ld=ld)
    torch.cuda.synchronize()
    assert float(planes.min()) < 0 and float(planes.max()) > 1
    return rows, base, planes


KERNEL = [(2, 12), (2, 48), (3, 28), (3, 48), (4, 48)]


def _crops(s, even):
    """The full image and a smaller crop; both even where the layout subsamples (x3: the full 15 x 21 image is then 14 x 20)."""
    H, W = s * LR[0], s * LR[1]
    if even:
        return [(H - H % 2, W - W % 2), (H - H % 2 - 4, W - W % 2 - 6)]
    return [(H, W), (H - 3, W - 5)]


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("s,ld", KERNEL, ids=[f"x{s}_ld{ld}" for s, ld in KERNEL])
def test_shuffle_to_u8_equals_shuffle_then_planes_to_u8(s, ld, with_base):
    """bgr off and on, the full image and a crop, and pitched rows (a slice of a wider tensor) whose other bytes stay 0xA5."""
    from super_resolution_amd import ops
    rows, base, planes = _source(s, ld, with_base)
    geo = dict(B=B, H=LR[0], W=LR[1], s=s, ld=ld)
    for h, w in _crops(s, False):
        for bgr in (False, True):
            want = torch.empty(B, h, w, 3, dtype=torch.uint8, device=rows.device)
            ops.planes_to_u8(planes, want, bgr=bgr)
            got = torch.full((B, h, w, 3), 0xA5, dtype=torch.uint8, device=rows.device)
            ops.shuffle_to_u8(rows, base, got, bgr=bgr, **geo)
            wide = torch.full((B, h + 2, w + 5, 3), 0xA5, dtype=torch.uint8, device=rows.device)
            ops.shuffle_to_u8(rows, base, wide[:, 1:h + 1, 2:w + 2], bgr=bgr, **geo)
            torch.cuda.synchronize()
            assert torch.equal(got, want), f"x{s} ld {ld} {h}x{w} bgr={bgr}: {int((got != want).sum())} bytes differ"
            assert torch.equal(wide[:, 1:h + 1, 2:w + 2], want)
            wide[:, 1:h + 1, 2:w + 2] = 0xA5
            assert bool((wide == 0xA5).all()), "the pitched sink wrote outside its rows"
    assert int(want.min()) == 0 and int(want.max()) == 255


YUV = [(f, 8, None) for f in ("i420", "nv12", "nv21", "i422", "nv16", "i444", "nv24", "gray")] + [("i420", 10, False), ("nv12", 10, True),
                                                                                                  ("i444", 10, False)]


def _frame_buffer(B_, hw, fmt, depth):
    from super_resolution_amd import yuv
    if depth == 8:
        return torch.full((B_,) + yuv.frame_shape_fmt(*hw, fmt), 0xA5, dtype=torch.uint8, device=_dev())
    return torch.full((B_,) + yuv.frame_shape_fmt(*hw, fmt), 0x5A5A, dtype=torch.int16, device=_dev()).view(torch.uint16)


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("fmt,depth,msb", YUV, ids=[f"{f}_{d}{'' if m is None else 'msb' if m else 'lsb'}" for f, d, m in YUV])
@pytest.mark.parametrize("s,ld", [(2, 12), (3, 28), (4, 48)], ids=["x2", "x3", "x4"])
def test_shuffle_to_yuv_equals_shuffle_then_planes_to_yuv(s, ld, fmt, depth, msb, with_base):
    """Every layout, centre-sited, the full image (where the layout allows its size) and a crop; the frame buffers start filled, so
    a sample the sink leaves out shows."""
    from super_resolution_amd import ops, yuv
    rows, base, planes = _source(s, ld, with_base)
    from_rgb = yuv.csc(depth=depth, **BT601)[1]
    msb = bool(yuv.container(depth, fmt, msb)[3])
    for hw in _crops(s, SUB[fmt] is not None and SUB[fmt] != (0, 0)):
        want, got = _frame_buffer(B, hw, fmt, depth), _frame_buffer(B, hw, fmt, depth)
        ops.planes_to_yuv(planes, *ops.yuv_views(want, fmt), from_rgb, sub=SUB[fmt], depth=depth, msb=msb)
        ops.shuffle_to_yuv(rows, base, *ops.yuv_views(got, fmt), from_rgb, B=B, H=LR[0], W=LR[1], s=s, ld=ld, sub=SUB[fmt], depth=depth, msb=msb)
        torch.cuda.synchronize()
        assert _eq(got, want), f"{fmt} x{s} {hw} depth {depth} msb {msb}: differs from planes_to_yuv"


def test_sinks_against_the_host_definition():
    """x3 with the base image: the bytes are tensor2img's of the planes, the i420 frame yuv.planes_to_yuv's, computed in numpy."""
    from super_resolution_amd import ops, yuv
    rows, base, planes = _source(3, 28, True)
    p = planes.cpu().numpy()
    got = torch.empty(B, 15, 21, 3, dtype=torch.uint8, device=rows.device)
    ops.shuffle_to_u8(rows, base, got, B=B, H=5, W=7, s=3, ld=28)
    want = np.rint(np.clip(p, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(got.cpu().numpy(), want)
    fr = _frame_buffer(B, (14, 20), "i420", 8)
    ops.shuffle_to_yuv(rows, base, *ops.yuv_views(fr, "i420"), yuv.csc(**BT601)[1], B=B, H=5, W=7, s=3, ld=28, sub=(1, 1))
    assert np.array_equal(fr.cpu().numpy(), yuv.planes_to_yuv(p[:, :, :14, :20], fmt="i420", **BT601))


def test_wrappers_refuse_before_any_launch():
    from super_resolution_amd import ops
    rows, base, _ = _source(2, 12, True)
    geo = dict(B=B, H=5, W=7, s=2, ld=12)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=rows.device)
    with pytest.raises(RuntimeError, match="destination"):
        ops.shuffle_to_u8(rows, base, u8(B, 11, 14, 3), **geo)
    with pytest.raises(RuntimeError, match="destination"):
        ops.shuffle_to_u8(rows, base, u8(B, 10, 14, 3).float(), **geo)
    with pytest.raises(RuntimeError, match="base image"):
        ops.shuffle_to_u8(rows, base[:, :, :4], u8(B, 10, 14, 3), **geo)
    with pytest.raises(RuntimeError, match="Y view"):
        ops.shuffle_to_yuv(rows, base, u8(B, 12, 14), None, None, [0.0] * 12, sub=None, **geo)


# ------------------------------------------------------------------------------------------------
# whole models, the weights and frames of the existing fixtures, the frames quantised to bytes
# ------------------------------------------------------------------------------------------------
MODELS = {"esc_a": (_esc_net, "a", 2), "escreal_b": (_escreal_net, "b", 4), "escreal_c": (_escreal_net, "c", None),
          "escrealm_a": (_escrealm_net, "a", None), "escrealm_b": (_escrealm_net, "b", None), "escfp_c": (_escfp_net, "c", None)}
FUSED_U8 = {"esc_a": True, "escrealm_b": True, "escreal_c": False, "escfp_c": False}   # the shuffle route; the two planes-only heads


def _model(key, dtype):
    mk, name, _ = MODELS[key]
    net, g, _ = mk(name, dtype, _dev())
    x = torch.from_numpy(np.asarray(g["x"], dtype=np.float32))
    frame = (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous().to(_dev())
    return net, frame


def _planes_of(frame, bgr=False):
    from super_resolution_amd import ops
    b, h, w, _ = frame.shape
    x = torch.empty(b, 3, h, w, device=frame.device)
    ops.u8_to_planes(frame, x, bgr=bgr)
    return x


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("key", list(MODELS))
def test_upscale_u8_is_the_composition(key, dtype):
    """upscale_u8(frame) == planes_to_u8(forward(u8_to_planes(frame))), and the counters show the route that ran."""
    from super_resolution_amd import ops
    net, frame = _model(key, dtype)
    S, eng = net.upscale, net.engine(frame.device)
    b, h, w, _ = frame.shape
    if MODELS[key][2] is not None:
        assert S == MODELS[key][2]          # escreal "b": x4 although upscaling_factor = 2
    if key == "escreal_b":
        assert int(net.cfg["upscaling_factor"]) == 2 and (4 * w) % 16 == 0
    for bgr in (False, True):
        want = torch.empty(b, S * h, S * w, 3, dtype=torch.uint8, device=frame.device)
        ops.planes_to_u8(net(_planes_of(frame, bgr)).contiguous(), want, bgr=bgr)
        before = (eng.u8_fused_calls, eng.u8_planes_calls)
        got = net.upscale_u8(frame, bgr=bgr)
        ran = (eng.u8_fused_calls - before[0], eng.u8_planes_calls - before[1])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (b, S * h, S * w, 3)
        assert torch.equal(got, want), f"{key} [{dtype}] bgr={bgr}: {int((got != want).sum())} of {want.numel()} bytes differ"
        if key in FUSED_U8:
            assert ran == ((1, 0) if FUSED_U8[key] else (0, 1)), (key, ran)
        elif key == "escreal_b":   # the conv route: the row sweep exists for bf16 rows only
            assert ran == ((1, 0) if dtype == "bf16" else (0, 1)), (key, dtype, ran)
    if b == 1:
        assert torch.equal(net.upscale_u8(frame[0]), net.upscale_u8(frame))   # (h,w,3) is one frame


def _yuv_in(frame, fmt, depth=8):
    """The byte frame's planes as a YCbCr frame of `fmt` (host definition), on the device."""
    from super_resolution_amd import yuv
    p = frame.permute(0, 3, 1, 2).float().div(255).cpu().numpy()
    return torch.from_numpy(yuv.planes_to_yuv(p, fmt=fmt, out_depth=depth, **BT601)).to(frame.device)


def _compose_yuv(net, fr, fmt, out_fmt, out_depth=8, out_siting="center"):
    from super_resolution_amd import ops, yuv
    h, w = yuv.frame_size_fmt(fr.shape, fmt)
    x = torch.empty(fr.shape[0], 3, h, w, device=fr.device)
    ops.yuv_to_planes(*ops.yuv_views(fr, fmt), x, yuv.csc(**BT601)[0], sub=SUB[fmt])
    y = net(x).contiguous()
    want = _frame_buffer(fr.shape[0], tuple(y.shape[2:]), out_fmt, out_depth)
    ops.planes_to_yuv(y, *ops.yuv_views(want, out_fmt), yuv.csc(depth=out_depth, **BT601)[1], sub=SUB[out_fmt], depth=out_depth,
                      msb=bool(yuv.container(out_depth, out_fmt, None)[3]), siting=out_siting)
    return want


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("key", list(MODELS))
def test_upscale_yuv_is_the_composition(key, dtype):
    net, frame = _model(key, dtype)
    eng = net.engine(frame.device)
    odd = frame.shape[1] % 2 or frame.shape[2] % 2
    cases = [("i444", "i444", 8)] if odd else [("nv12", "nv12", 8), ("i420", "i444", 10)]
    for fmt, out_fmt, out_depth in cases:
        fr = _yuv_in(frame, fmt)
        want = _compose_yuv(net, fr, fmt, out_fmt, out_depth)
        before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
        got = net.upscale_yuv(fr, fmt=fmt, out_fmt=out_fmt, out_depth=out_depth)
        ran = (eng.yuv_fused_calls - before[0], eng.yuv_planes_calls - before[1])
        assert _eq(got, want), f"{key} [{dtype}] {fmt} -> {out_fmt}: differs from the composition"
        if key in FUSED_U8:
            assert ran == ((1, 0) if FUSED_U8[key] else (0, 1)), (key, ran)
    if odd:   # escrealm "a", 67 x 81: nv12 on its 66 x 80 crop
        crop = frame[:, :frame.shape[1] - frame.shape[1] % 2, :frame.shape[2] - frame.shape[2] % 2].contiguous()
        fr = _yuv_in(crop, "nv12")
        assert _eq(net.upscale_yuv(fr, fmt="nv12"), _compose_yuv(net, fr, "nv12", "nv12"))
        with pytest.raises(RuntimeError, match="nv12 frames .* need an even width, got 66x81"):   # an odd-sized 4:2:0 frame is refused
            net.upscale_yuv(torch.zeros(1, 99, 81, dtype=torch.uint8, device=frame.device), fmt="nv12")


def test_a_co_sited_output_ends_in_planes():
    net, frame = _model("esc_a", "bf16")
    eng = net.engine(frame.device)
    fr = _yuv_in(frame, "i420")
    before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
    got = net.upscale_yuv(fr, fmt="i420", out_siting="left")
    assert (eng.yuv_fused_calls - before[0], eng.yuv_planes_calls - before[1]) == (0, 1)
    assert _eq(got, _compose_yuv(net, fr, "i420", "i420", out_siting="left"))


def test_fp32_bytes_against_the_cpu_restatement():
    """tests/esc_ref.forward on frame / 255, converted with tensor2img's rule: no byte more than one level away (the fp32 bar of
    1e-4 is 0.026 of a byte step: only rounding ties can move).  The bf16 bar stays on the float outputs in tests/test_gpu_esc.py."""
    net, frame = _model("esc_a", "fp32")
    cfg, sd, _, _ = esc_ref.load_case("a")
    x = frame.cpu().permute(0, 3, 1, 2).double() / 255
    ref = esc_ref.forward(esc_ref.d64(sd), cfg, x)
    want = (ref.clamp(0, 1).float() * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1)
    diff = (net.upscale_u8(frame).cpu().int() - want.int()).abs()
    print(f"ESC a upscale_u8 vs the restatement: {float((diff != 0).float().mean()):.5f} of {diff.numel()} bytes differ, max {int(diff.max())}")
    assert int(diff.max()) <= 1


@pytest.mark.parametrize("key", ["esc_a", "escrealm_a"])
def test_upscale_ensemble_is_the_composition(key):
    """escrealm "a": the transposed members run an 81 x 67 frame behind the unshuffled stem."""
    net, frame = _model(key, "bf16")
    x = _planes_of(frame)
    ref = E.ensemble(net, x, 8)
    got = net.upscale_ensemble(x, 8)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and torch.equal(got, ref)
    assert torch.equal(net.upscale_ensemble(x, 1), net(x))


@pytest.mark.parametrize("key", ["esc_a", "escrealm_a"])
def test_byte_paths_with_the_ensemble(key):
    from super_resolution_amd import ops
    net, frame = _model(key, "bf16")
    S, (b, h, w, _) = net.upscale, frame.shape
    want = torch.empty(b, S * h, S * w, 3, dtype=torch.uint8, device=frame.device)
    ops.planes_to_u8(net.upscale_ensemble(_planes_of(frame), 4).contiguous(), want)
    assert torch.equal(net.upscale_u8(frame, ensemble=4), want)
    assert torch.equal(net.upscale_to_u8(_planes_of(frame), ensemble=4, crop=(S * h - 3, S * w - 5)), want[:, :S * h - 3, :S * w - 5])


def test_imresize_takes_a_pad_of_zero():
    """What upscale_gt_u8 asks of ops.imresize with nothing to pad: dst= the staging buffer and pad_to= the resized size itself."""
    from super_resolution_amd import ops
    gt = torch.randint(0, 256, (1, 80, 96, 3), dtype=torch.uint8, device=_dev(), generator=torch.Generator(_dev()).manual_seed(7))
    want = ops.imresize(gt, 0.25)
    dst = torch.full((1, 3, 20, 24), float("nan"), device=gt.device)
    assert ops.imresize(gt, 0.25, dst=dst, pad_to=(20, 24)) is dst and torch.equal(dst, want)


@pytest.mark.parametrize("ensemble", [1, 4])
@pytest.mark.parametrize("key,gt_hw,S", [("esc_a", (81, 97), 2), ("escreal_b", (83, 99), 4)], ids=["esc_a", "escreal_b"])
def test_upscale_gt_u8_is_the_composition(key, gt_hw, S, ensemble):
    """upscale_gt_u8(gt) == planes_to_u8(forward(imresize(mod-cropped gt, 1 / S))), the ensemble's likewise.  escreal "b": the
    low-resolution image is made at 1/4 although upscaling_factor = 2 (the default head is x4); the frame is not padded, so
    imresize writes a staging buffer of the resized size itself."""
    from super_resolution_amd import ops
    net, _ = _model(key, "bf16")
    dev = _dev()
    assert net.upscale == S
    gt = torch.randint(0, 256, (1,) + gt_hw + (3,), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(gt_hw[0]))
    H, W = gt_hw[0] - gt_hw[0] % S, gt_hw[1] - gt_hw[1] % S
    for bgr in (False, True):
        x = ops.imresize(gt[:, :H, :W], 1.0 / S, bgr=bgr)
        assert tuple(x.shape) == (1, 3, H // S, W // S)
        y = net(x) if ensemble == 1 else net.upscale_ensemble(x, ensemble)
        want = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
        ops.planes_to_u8(y.contiguous(), want, bgr=bgr)
        got = net.upscale_gt_u8(gt, bgr=bgr, ensemble=ensemble)
        assert tuple(got.shape) == (1, H, W, 3) and torch.equal(got, want), f"{key} bgr={bgr} ensemble={ensemble}: {int((got != want).sum())} bytes differ"
    assert torch.equal(net.upscale_gt_u8(gt[0], ensemble=ensemble), net.upscale_gt_u8(gt, ensemble=ensemble))   # (H,W,3) is one frame


def test_the_ensemble_with_out_allocates_nothing_on_the_second_call():
    """escrealm "a": every member's image is a corner of the x4 buffer, copied into the member's workspace, not into a fresh tensor."""
    net, frame = _model("escrealm_a", "bf16")
    dev, S, (b, h, w, _) = frame.device, net.upscale, frame.shape
    out = torch.empty(b, S * h, S * w, 3, dtype=torch.uint8, device=dev)
    first = net.upscale_u8(frame, out=out, ensemble=8).clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert net.upscale_u8(frame, out=out, ensemble=8) is out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before, "upscale_u8(ensemble=8, out=) allocated on its second run"
    assert torch.equal(out, first)


def test_out_tensors_and_no_allocation_on_the_second_call():
    net, frame = _model("esc_a", "bf16")
    dev, S, (b, h, w, _) = frame.device, net.upscale, frame.shape
    fr = _yuv_in(frame, "i420")
    out_u8 = torch.empty(b, S * h, S * w, 3, dtype=torch.uint8, device=dev)
    out_yv = torch.empty(b, 3 * S * h // 2, S * w, dtype=torch.uint8, device=dev)
    first = (net.upscale_u8(frame, out=out_u8).clone(), net.upscale_yuv(fr, fmt="i420", out=out_yv).clone())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    assert net.upscale_u8(frame, out=out_u8) is out_u8
    assert net.upscale_yuv(fr, fmt="i420", out=out_yv) is out_yv
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before, "a call with out= allocated on its second run"
    assert torch.equal(out_u8, first[0]) and torch.equal(out_yv, first[1])
    with pytest.raises(RuntimeError, match="out must be"):
        net.upscale_u8(frame, out=out_u8[:, :-1])
    with pytest.raises(RuntimeError, match="out must be"):
        net.upscale_yuv(fr, fmt="i420", out=out_u8)


def test_frame_refusals():
    net, frame = _model("esc_a", "bf16")
    dev = frame.device
    with pytest.raises(RuntimeError, match="one frame"):
        net.upscale_u8(torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="reflect-padded"):   # (-16) % 32 = 16 > 15: the reflection is larger than the frame
        net.upscale_u8(torch.zeros(16, 24, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="i420 frames .* need an even width, got 22x21"):
        net.upscale_yuv(torch.zeros(1, 33, 21, dtype=torch.uint8, device=dev), fmt="i420")
    with pytest.raises(RuntimeError, match=r"a i420 frame is a \(3h/2, w\) array"):   # (an odd height has no 4:2:0 array at all)
        net.upscale_yuv(torch.zeros(1, 31, 22, dtype=torch.uint8, device=dev), fmt="i420")
    with pytest.raises(RuntimeError, match="uint8"):
        net.upscale_u8(torch.zeros(1, 20, 24, 3, device=dev))
    assert tuple(net.upscale_u8(torch.zeros(20, 24, 3, dtype=torch.uint8, device=dev)).shape) == (1, 40, 48, 3)


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
def _toy_opt(tmp_path, ref, arch, case, scale, **extra):
    import yaml
    cfg, sd, _, _ = ref.load_case(case)
    torch.save({"params": sd}, tmp_path / "net.pth")
    opt = {"name": "toy", "model_type": "ESRModel", "scale": scale, "num_gpu": 1,
           "network_g": dict(cfg, type=arch, attn_type="Naive", compute_dtype="bf16"),
           "path": {"pretrain_network_g": str(tmp_path / "net.pth"), "strict_load_g": True, "param_key_g": "params",
                    "visualization": str(tmp_path / "vis")}}
    opt.update(extra)
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    return str(tmp_path / "opt.yml")


def test_video_tool_on_a_toy_escreal(tmp_path):
    """A 3-frame 20 x 24 Y4M through `python -m super_resolution_amd.video` with an ESCReal option file: a Y4M of 80 x 96 whose frames
    are upscale_frames' (and through it upscale_yuv's)."""
    _dev()
    from super_resolution_amd import frames, video, y4m
    from super_resolution_amd.models import HATModel
    from super_resolution_amd.test import parse_options
    opt = _toy_opt(tmp_path, escreal_ref, "ESCReal", "a", 4)
    rng = np.random.default_rng(5)
    src = [rng.integers(16, 236, (30, 24), dtype=np.uint8) for _ in range(3)]
    with y4m.Writer(str(tmp_path / "in.y4m"), dict(W=24, H=20, F="25:1", C="420jpeg"), chroma=True) as wr:
        for f in src:
            wr.write(f)
    info = video.main(["-opt", opt, "-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.y4m")])
    assert info["frames"] == 3 and info["out"] == (96, 80)
    model = HATModel(parse_options(opt), device="cuda:0")
    want = list(frames.upscale_frames(model.get_bare_model(model.net_g), src, pixfmt="i420"))
    with y4m.Reader(str(tmp_path / "out.y4m"), chroma=True) as rd:
        got = list(rd)
        assert (rd.w, rd.h) == (96, 80)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_harness_u8_and_metrics_on_device_on_a_toy_esr_model(tmp_path):
    """`python -m super_resolution_amd.test` on an ESRModel option file (ESC x2): with val.u8_on_device + val.metrics_on_device it
    writes the PNGs its float run writes, byte for byte (the byte branch pads as the float branch does and ends in the same
    conversion), and its device scores are the float run's host scores within 1e-8 dB / 1e-10 SSIM, the bars tests/test_gpu_metrics.py
    and tests/test_gpu_ensemble.py hold hat_u8_metrics to on equal images."""
    _dev()
    from super_resolution_amd import data as D, metrics as M, synth, test as T
    for i, (h, w) in enumerate([(40, 46), (36, 50)]):
        gt = synth.synth_input(40 + i, (1, 3, 2 * h, 2 * w))
        D.write_image(M.tensor2img(gt), str(tmp_path / "gt" / f"im{i}.png"))
        D.write_image(M.tensor2img(torch.nn.functional.avg_pool2d(gt, 2)), str(tmp_path / "lq" / f"im{i}.png"))
    ds = {"test_1": {"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"), "dataroot_lq": str(tmp_path / "lq"),
                     "io_backend": {"type": "disk"}}}
    metrics = {"psnr": {"type": "calculate_psnr", "crop_border": 2, "test_y_channel": True},
               "ssim": {"type": "calculate_ssim", "crop_border": 2, "test_y_channel": True}}
    res = {}
    for mode, val in (("float", {}), ("u8", {"u8_on_device": True, "metrics_on_device": True})):
        sub = tmp_path / mode
        sub.mkdir()
        opt = _toy_opt(sub, esc_ref, "ESC", "a", 2, datasets=ds, val=dict(save_img=True, suffix=None, metrics=metrics, **val))
        res[mode] = T.main(["-opt", opt])["Toy"]
    for i in range(2):
        a = D.read_image(str(tmp_path / "float" / "vis" / "Toy" / f"im{i}_toy.png"))
        b = D.read_image(str(tmp_path / "u8" / "vis" / "Toy" / f"im{i}_toy.png"))
        assert a.shape == b.shape and torch.equal(a, b), f"im{i}: the byte run's PNG differs from the float run's"
        fa, fb = res["float"]["images"][i], res["u8"]["images"][i]
        assert abs(fa["psnr"] - fb["psnr"]) <= 1e-8 and abs(fa["ssim"] - fb["ssim"]) <= 1e-10, (fa, fb)


def test_harness_tiled_self_ensemble_and_lq_on_device_on_a_toy_esr_model(tmp_path):
    """The other byte branches of the harness on an ESRModel option file (ESC x2): the tiled branch and val.self_ensemble write the
    PNG their float runs write, byte for byte; val.lq_on_device writes the bytes of its composition — ops.imresize of the mod-cropped
    ground truth into the padded planes, `forward`, the crop, hat_planes_to_u8."""
    dev = _dev()
    from super_resolution_amd import data as D, metrics as M, ops, synth, test as T
    h, w = 40, 46
    gt = synth.synth_input(47, (1, 3, 2 * h + 1, 2 * w))
    D.write_image(M.tensor2img(gt), str(tmp_path / "gt" / "im0.png"))
    D.write_image(M.tensor2img(torch.nn.functional.avg_pool2d(gt[:, :, :2 * h], 2)), str(tmp_path / "lq" / "im0.png"))
    ds = {"test_1": {"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"), "dataroot_lq": str(tmp_path / "lq"),
                     "io_backend": {"type": "disk"}}}
    png = lambda mode: D.read_image(str(tmp_path / mode / "vis" / "Toy" / "im0_toy.png"))

    def run(mode, val, **extra):
        (tmp_path / mode).mkdir()
        T.main(["-opt", _toy_opt(tmp_path / mode, esc_ref, "ESC", "a", 2, datasets=ds, val=dict(save_img=True, suffix=None, **val), **extra)])

    tile = {"tile": {"tile_size": 32, "tile_pad": 8}}
    for name, val, extra in (("tile", {}, tile), ("ens", {"self_ensemble": 4}, {}), ("tile_ens", {"self_ensemble": 2}, tile)):
        run(name + "_float", val, **extra)
        run(name + "_u8", dict(val, u8_on_device=True), **extra)
        a, b = png(name + "_float"), png(name + "_u8")
        assert tuple(a.shape) == (3, 2 * h, 2 * w) and torch.equal(a, b), f"{name}: the byte run's PNG differs from the float run's"
    assert not torch.equal(png("ens_float"), png("tile_float"))
    run("lq_dev", {"lq_on_device": True, "metrics_on_device": True})
    net, _ = _model("esc_a", "bf16")
    gt8 = torch.from_numpy(M.tensor2img(D.read_image(str(tmp_path / "gt" / "im0.png")).unsqueeze(0)).copy()).unsqueeze(0).to(dev)
    x = ops.imresize(gt8[:, :2 * h], 0.5, pad_to=(64, 64))
    want = torch.empty(1, 2 * h, 2 * w, 3, dtype=torch.uint8, device=dev)
    ops.planes_to_u8(net(x).contiguous(), want)
    got = torch.from_numpy(M.tensor2img(png("lq_dev").unsqueeze(0)).copy())
    assert torch.equal(got, want[0].cpu()), "val.lq_on_device: the PNG differs from imresize -> forward -> crop -> planes_to_u8"
