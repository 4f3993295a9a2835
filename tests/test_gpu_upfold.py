"""The folded ending of the network on the GPU (hat_upfold_*): the last PixelShuffle(2) conv and conv_last as one 5x5
conv.  The kernel against the fp64 composition, no worse than the two launches it replaces; every sink form equal to
planes-then-convert; the engine launches it where it should, and plans record and replay it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import META, W_SEED, X_SEED
from super_resolution_amd import synth, yuv

pytestmark = pytest.mark.gpu
MEAN, SCALE = (0.4488, 0.4371, 0.4040), 0.5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _layer(seed, B, H, W, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, 64, generator=g).to(torch.bfloat16)
    wu, bu = torch.randn(256, 64, 3, 3, generator=g) / 24.0, torch.randn(256, generator=g) * 0.1
    wl, bl = torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0), torch.randn(3, generator=g) * 0.1
    return x.to(dev), x, (wu, bu, wl, bl)


def _reference(x, wu, bu, wl, bl):
    """conv -> pixel_shuffle -> conv in fp64 on the bf16 input, unrounded weights, then conv_last's scale and mean."""
    d = lambda t: t.to(torch.float64)
    y = F.conv2d(F.pixel_shuffle(F.conv2d(d(x).permute(0, 3, 1, 2), d(wu), d(bu), padding=1), 2), d(wl), d(bl), padding=1)
    return y * SCALE + torch.tensor(MEAN, dtype=torch.float64)[None, :, None, None]


# smallest width with 1, 2, 3 rows; one tile with partial rows; two trips of the persistent loop (B = 2: 128 workgroups a sample,
# 130 tiles) whose last tile is half as wide
SHAPES = [(1, 16), (2, 16), (3, 16), (11, 32), (3, 4144)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_folded_kernel_is_no_worse_than_the_two_launches(shape):
    dev = _dev()
    from super_resolution_amd import _lib, ops, packing
    H, W = shape
    B = 2
    xd, x, w = _layer(100 + H + W, B, H, W, dev)
    ref = _reference(x, *w)
    kw = dict(B=B, out_scale=SCALE, mean=MEAN, dtype=ops.HAT_BF16)
    got = torch.full((B, 3, 2 * H, 2 * W), 7.0, device=dev)
    ops.upfold_to_planes(xd, ops.pack_upfold(*w, dev), got, H=H, W=W, ldx=64, **kw)
    # the planes entry itself (ops goes through hat_conv's out_mode O_FOLD2_NCHW_F32, the form plans record): the same bits
    direct = torch.full_like(got, 3.0)
    pf = ops.pack_upfold(*w, dev)
    _lib.check(_lib.load().hat_upfold_to_planes(xd.data_ptr(), pf.w.data_ptr(), pf.bias.data_ptr(), direct.data_ptr(), B, H, W, 64, SCALE, *MEAN,
                                                ops.HAT_BF16, torch.cuda.current_stream().cuda_stream), "hat_upfold_to_planes")
    torch.cuda.synchronize()
    assert torch.equal(direct, got)
    # today's two launches on the same inputs
    mid = torch.zeros(B, 4 * H * W, 64, dtype=torch.bfloat16, device=dev)
    ops.conv(packing.pack_pixshuf_conv(w[0], w[1], 2, ops.HAT_BF16, dev), xd, mid, B=B, H=H, W=W, dtype=ops.HAT_BF16, ldx=64, ldo=64,
             out_mode=ops.O_PIXSHUF_T, ps_r=2)
    two = torch.empty_like(got)
    ops.conv3x3_to_planes(mid, *ops.pack_cab_squeeze(w[2], w[3], dev), two, H=2 * H, W=2 * W, C_=64, ldx=64, n_out=3, **kw)
    torch.cuda.synchronize()
    ef, et = got.cpu().double() - ref, two.cpu().double() - ref
    stats = lambda e: (float(e.abs().max()), float(e.pow(2).mean().sqrt()))
    (fm, fr), (tm, tr) = stats(ef), stats(et)
    print(f"upfold {H}x{W}: folded max-abs {fm:.3e} rms {fr:.3e} | two launches max-abs {tm:.3e} rms {tr:.3e}")
    assert fm <= tm and fr <= tr
    # the border ring on its own: no worse there either (a wrong border rule would be an error of the size of the values)
    ring = torch.ones(2 * H, 2 * W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert float(ef[..., ring].abs().max()) <= tm


def _sub(fmt):
    return None if yuv.LAYOUTS[fmt][0] is None else yuv.LAYOUTS[fmt][:2]


def _empty(B, h, w, fmt, depth, dev, fill):
    t = torch.full((B,) + yuv.frame_shape_fmt(h, w, fmt), fill, dtype=(torch.uint8 if depth == 8 else torch.int16), device=dev)
    return t if depth == 8 else t.view(torch.uint16)


def _n(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


# (H, W) of the folded conv's input: border-only frames, partial tile rows, several tiles and two trips
SINK_SHAPES = [(1, 16), (9, 48), (19, 2080)]


@pytest.mark.parametrize("shape", SINK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upfold_sinks_equal_planes_then_convert(shape):
    dev = _dev()
    from super_resolution_amd import ops
    H, W = shape
    B, Ho, Wo = 2, 2 * shape[0], 2 * shape[1]
    xd, _, w = _layer(7 + W, B, H, W, dev)
    pf = ops.pack_upfold(*w, dev)
    kw = dict(B=B, H=H, W=W, ldx=64, out_scale=SCALE, mean=MEAN, dtype=ops.HAT_BF16)
    planes = torch.empty(B, 3, Ho, Wo, device=dev)
    ops.upfold_to_planes(xd, pf, planes, **kw)
    for bgr in (False, True):
        for ho, wo in ((Ho, Wo), (Ho - 1, Wo - 5), (1, 1)):
            ref, out = (torch.full((B, ho, wo, 3), f, dtype=torch.uint8, device=dev) for f in (77, 55))
            ops.planes_to_u8(planes, ref, bgr=bgr)
            ops.upfold_to_u8(xd, pf, out, h_out=ho, w_out=wo, bgr=bgr, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (bgr, ho, wo)
    for fmt in ("i420", "nv12", "i422", "nv16", "i444", "nv24", "gray"):
        sx, sy, _ = yuv.LAYOUTS[fmt]
        for depth in (8, 10):
            msb = bool(yuv.container(depth, fmt)[3])
            m = yuv.csc("bt709", True, depth)[1]
            for ho, wo in ((Ho, Wo), (max(Ho - 3 + (sy == 1), 1 + (sy == 1)), Wo - 5 + (sx == 1)), (1 + (sy == 1), 1 + (sx == 1))):
                ref, out = _empty(B, ho, wo, fmt, depth, dev, 77), _empty(B, ho, wo, fmt, depth, dev, 55)
                ops.planes_to_yuv(planes, *ops.yuv_views(ref, fmt), m, sub=_sub(fmt), depth=depth, msb=msb)
                ops.upfold_to_yuv(xd, pf, *ops.yuv_views(out, fmt), sub=_sub(fmt), from_rgb=m, depth=depth, msb=msb, **kw)
                torch.cuda.synchronize()
                assert np.array_equal(_n(out), _n(ref)), (fmt, depth, ho, wo)


def test_upfold_refuses_what_it_is_not_built_for():
    dev = _dev()
    from super_resolution_amd import ops
    xd, _, w = _layer(1, 1, 2, 24, dev)
    pf = ops.pack_upfold(*w, dev)
    with pytest.raises(RuntimeError):      # W % 16
        ops.upfold_to_planes(xd, pf, torch.empty(1, 3, 4, 48, device=dev), B=1, H=2, W=24, ldx=64, out_scale=1.0, mean=MEAN, dtype=ops.HAT_BF16)
    with pytest.raises(RuntimeError):      # the fp32 path keeps the two launches
        ops.upfold_to_planes(xd, pf, torch.empty(1, 3, 4, 32, device=dev), B=1, H=2, W=16, ldx=64, out_scale=1.0, mean=MEAN, dtype=ops.HAT_F32)
    with pytest.raises(RuntimeError):      # a destination of another size
        ops.upfold_to_planes(xd, pf, torch.empty(1, 3, 4, 30, device=dev), B=1, H=2, W=16, ldx=64, out_scale=1.0, mean=MEAN, dtype=ops.HAT_BF16)


def _net(name, dtype, dev):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(type="HAT", compute_dtype=dtype, **META["cfgs"][name])).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    return net.to(dev)


def _launches(net, x):
    from super_resolution_amd import ops
    with ops.profile() as rec:
        y = net(x)
        torch.cuda.synchronize()
    return y, [r[0] for r in rec]


@pytest.mark.parametrize("case", [("hats_1g_x4", (1, 3, 16, 32)), ("hat_1g_x2", (2, 3, 16, 16))], ids=lambda c: c[0])
def test_engine_ends_folded_on_the_bf16_path_and_plans_replay_it(case, tmp_path):
    dev = _dev()
    from super_resolution_amd import metrics, ops, plan
    name, shape = case
    net = _net(name, "bf16", dev)
    x = synth.synth_input(X_SEED + 3, shape).to(dev)
    y, names = _launches(net, x)
    y = y.clone()
    assert names[-1] == "upfold_kernel<planes>" and not any(n.startswith("cab_squeeze_kernel<2") for n in names)
    s = META["cfgs"][name]["upscale"]
    eng = net.engine()
    assert eng.upfold is not None and eng._workspace(*shape[:1], *shape[2:])["ups"][-1] is None
    # bytes: the folded sink, equal to tensor2img of the planes
    before = (eng.u8_fused_calls, eng.u8_planes_calls)
    y8 = net.forward_to_u8(x)
    assert (eng.u8_fused_calls, eng.u8_planes_calls) == (before[0] + 1, before[1])
    ref8 = np.stack([metrics.tensor2img(y[i].cpu()) for i in range(y.shape[0])])
    assert np.array_equal(y8.cpu().numpy(), ref8)
    # The plan records the folded ending — as the hat_conv call the engine makes, out_mode O_FOLD2_NCHW_F32 — and nothing changes
    # in the module: it still ends folded, and the replay equals it through every way out
    path = str(tmp_path / "net.hatplan")
    dims, buffers, calls = plan.record_plan(net, shape)
    name_last, args_last = calls[-1]
    desc = ops.HatConvDesc.from_buffer_copy(args_last[0][1])
    assert name_last == "hat_conv" and desc.out_mode == ops.O_FOLD2_NCHW_F32 and desc.ksize == 5
    info = plan.export_plan(net, shape, path)
    assert "hat_conv3x3_to_planes" not in info["functions"] and eng.upfold is not None and net.engine() is eng
    y2, names = _launches(net, x)
    assert names[-1] == "upfold_kernel<planes>" and torch.equal(y2, y)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    yp = torch.zeros_like(y)
    p.forward(x, yp, stream)
    torch.cuda.synchronize()
    assert torch.equal(yp, y)
    B, h, w = shape[0], shape[2] - 2, shape[3] - 2
    frames = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(dev)
    out = torch.zeros(B, s * h, s * w, 3, dtype=torch.uint8, device=dev)
    p.forward_u8(frames, out, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(out, net.forward_u8(frames))
    for fmt in ("nv12", "i444"):
        src = torch.randint(16, 236, (B,) + yuv.frame_shape_fmt(h, w, fmt), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(dev)
        want = net.forward_yuv(src, fmt=fmt)
        dst = torch.zeros_like(want)
        p.forward_yuv(src, dst, fmt=fmt, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(dst, want), fmt
    # a rebuilt engine (the module moved: HAT.engine() packs again) ends folded again and still equals the plan
    net.to(dev)
    net.mark_weights_changed()
    assert net.engine() is not eng and net.engine().upfold is not None
    p.forward(x, yp.zero_(), stream)
    torch.cuda.synchronize()
    assert torch.equal(net(x), yp)
    p.close()


@pytest.mark.parametrize("case", [("tiny_x3", "bf16", (1, 3, 16, 16)), ("hats_1g_x4", "f32", (1, 3, 16, 16)), ("tiny_x2", "bf16", (1, 3, 8, 24))],
                         ids=lambda c: f"{c[0]}-{c[1]}")
def test_engine_keeps_the_two_launches_elsewhere(case):
    """x3, the fp32 path, and a width the folded kernel does not take (24 columns into the last stage)."""
    dev = _dev()
    name, dtype, shape = case
    net = _net(name, dtype, dev)
    _, names = _launches(net, synth.synth_input(X_SEED, shape).to(dev))
    assert not any(n.startswith("upfold_kernel") for n in names)
    assert net.engine()._workspace(shape[0], *shape[2:])["ups"][-1] is not None
