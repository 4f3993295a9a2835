"""SRVGGNetCompact on the device.  hat_vgg_conv: exact-lattice parity (tests/srvgg_lattice.py: the fp64 reference rounded once to T, bit
for bit) in bf16 and fp32, in both input modes, on frames below, at and across the 16 x 16 tile and on the smallest frame at which the
kernel's own schedule gives one workgroup two trips; float parity of the same launches on random data; a mid-body tap and the whole
model against the reference's goldens (tests/golden/srvgg_*.npz, gen_golden_srvgg.py); eager against graph replay; the frame paths
against the two-step composition over this build's `forward`, bit for bit; and the fixture option file through the test harness.

Bars: fp32 1e-4 max-abs (the project's fp32 bar).  bf16 kernels: helpers.check's bar.  bf16 whole model, on the residual y - nearest(x):
the reference's own bf16 PSNR of the residual rounded down to a whole dB and capped at 40, and its max-abs x 1.25 (srvgg_surface.json;
40 dB / 0.08 where the recorded deviation is not finite), as for ESCReal."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ensemble_ref as E
import lattice as L
import srvgg_lattice as VL
import srvgg_ref as R
from helpers import check, max_abs, pads_keep, q, rnd
from oracle import hat_oracle as O

pytestmark = pytest.mark.gpu

LDO = 72          # rows of 64 live channels and 8 pad channels: 16-byte rows in both dtypes
BT601 = dict(matrix="bt601", full_range=False)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _launch(x, w, bias, slope, geom, mode, dtype, dev):
    """One hat_vgg_conv launch on host operands: x (B,H,W,cin) -> the raw (B, H W, LDO) output rows, pre-filled with L.FILL."""
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = geom
    pv = ops.pack_vgg_conv(w, bias, slope, dt, dev)
    if mode == "frame":
        xin, ldx = x.permute(0, 3, 1, 2).to(torch.float32).contiguous().to(dev), 0
    else:
        ldx = LDO
        xin = torch.full((B, H * W, ldx), L.POISON, dtype=tdt, device=dev)
        xin[:, :, :64] = x.reshape(B, H * W, 64).to(dev).to(tdt)
    out = torch.full((B, H * W, LDO), L.FILL, dtype=tdt, device=dev)
    ops.vgg_conv(pv, xin, out, B=B, H=H, W=W, dtype=dt, ldx=ldx, ldo=LDO)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _two_trip(dtype):
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    geom = VL.two_trip_geom(lambda B, H, W: ops.vgg_conv_tiles(B, H, W, dt))
    tiles, wgs, _ = ops.vgg_conv_tiles(*geom, dt)
    t = VL.trips(tiles, wgs)
    assert max(t) == 2 and min(t) == 1, (geom, tiles, wgs)
    return geom


GEOM_IDS = [f"{b}x{h}x{w}" for b, h, w in VL.GEOMS] + ["two_trips"]


@pytest.mark.parametrize("gi", range(len(VL.GEOMS) + 1), ids=GEOM_IDS)
@pytest.mark.parametrize("mode", VL.MODES)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_vgg_conv_exact_on_the_lattice(dtype, mode, gi):
    dev = _dev()
    geom = VL.GEOMS[gi] if gi < len(VL.GEOMS) else _two_trip(dtype)
    c = VL.vgg_case(geom, mode, dtype)
    out = _launch(c.x, c.w, c.bias, c.slope, geom, mode, dtype, dev)
    B, H, W = geom
    pads_keep(out, 64, L.FILL, f"hat_vgg_conv {mode} {geom} [{dtype}]")
    L.assert_bits(out[:, :, :64].reshape(B, H, W, 64), L.expect(c.ref, L.STORE[dtype]), f"hat_vgg_conv {mode} {geom} [{dtype}]")


@pytest.mark.parametrize("gi", range(len(VL.GEOMS) + 1), ids=GEOM_IDS)
@pytest.mark.parametrize("mode", VL.MODES)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_vgg_conv_matches_fp64_on_random_data(dtype, mode, gi):
    dev = _dev()
    geom = VL.GEOMS[gi] if gi < len(VL.GEOMS) else _two_trip(dtype)
    B, H, W = geom
    cin = 3 if mode == "frame" else 64
    key = f"vggr.{mode}.{geom}"
    x = q(rnd(key + "x", (B, H, W, cin)), dtype)
    w = q(rnd(key + "w", (64, cin, 3, 3), std=(9 * cin) ** -0.5), dtype)
    bias, slope = rnd(key + "b", (64,), std=0.1), rnd(key + "s", (64,), std=0.5)
    out = _launch(x, w, bias, slope, geom, mode, dtype, dev)
    want = R.act(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), padding=1), slope.double()).permute(0, 2, 3, 1)
    assert float((want < 0).double().mean()) > 0.1 or want.numel() < 4096
    pads_keep(out, 64, L.FILL, f"hat_vgg_conv {mode} {geom} [{dtype}]")
    got = out[:, :, :64].float().reshape(B, H, W, 64)
    if dtype == "f32":      # the absolute bar, whatever the reference's magnitude
        err = max_abs(got.cpu(), want)
        print(f"hat_vgg_conv {mode} {geom} [f32]: max-abs {err:.3e} (max |ref| {float(want.abs().max()):.2f})")
        assert torch.isfinite(got).all() and err <= 1e-4, f"hat_vgg_conv {mode} {geom} [f32]: max-abs {err:.3e}"
    else:
        check(got, want, dtype, f"hat_vgg_conv {mode} {geom}")


def test_vgg_conv_wrapper_refuses_before_any_launch():
    dev = _dev()
    from super_resolution_amd import ops
    pv = ops.pack_vgg_conv(rnd("rw", (64, 64, 3, 3)), rnd("rb", (64,)), rnd("rs", (64,)), ops.HAT_F32, dev)
    x, out = torch.zeros(1, 35, 64, device=dev), torch.full((1, 35, 64), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.vgg_conv(pv, x, x, B=1, H=5, W=7, dtype=ops.HAT_F32)                 # out == x
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.vgg_conv(pv, x, out, B=1, H=5, W=7, dtype=ops.HAT_F32, ldo=62)
    with pytest.raises(RuntimeError, match="packed for"):
        ops.vgg_conv(pv, x, out, B=1, H=5, W=7, dtype=ops.HAT_BF16)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0, "a refused call launched"


# ---- whole model ------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name, dtype, dev):
    from super_resolution_amd.registry import build_network
    if (name, dtype) not in _NETS:
        cfg, sd, g, meta = R.load_case(name)
        net = build_network(dict(cfg, type="SRVGGNetCompact", compute_dtype=dtype)).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[(name, dtype)] = (net.to(dev), g, meta)
    return _NETS[(name, dtype)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mid_body_tap_matches_the_reference_rows(dtype):
    dev = _dev()
    net, g, _ = _net(R.TAP_CASE, dtype, dev)
    taps = {}
    net.engine(dev).forward(torch.from_numpy(g["x"]).to(dev), taps=taps)
    torch.cuda.synchronize()
    assert sorted(taps) == list(range(net.num_conv + 1))
    got = taps[R.TAP_LAYER][0].float().cpu()[torch.from_numpy(g["tap_pixels"])]
    want = torch.from_numpy(g["tap"])
    if dtype == "fp32":     # the project's fp32 bar, absolute
        err = max_abs(got, want)
        print(f"srvgg_{R.TAP_CASE} layer {R.TAP_LAYER} [fp32]: max-abs {err:.3e}")
        assert torch.isfinite(got).all() and err <= 1e-4, f"srvgg_{R.TAP_CASE} layer {R.TAP_LAYER} [fp32]: max-abs {err:.3e}"
    else:
        check(got, want, "bf16", f"srvgg_{R.TAP_CASE} layer {R.TAP_LAYER} [bf16]")


@pytest.mark.parametrize("name", list(R.CASES))
def test_whole_model_fp32_matches_reference(name):
    dev = _dev()
    net, g, meta = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    y = net(x)
    assert list(y.shape) == meta["out"]
    err = max_abs(y.cpu(), g["y"])
    print(f"srvgg_{name} y: max-abs {err:.3e}")
    assert err <= 1e-4, f"srvgg_{name}: max-abs {err:.3e}"
    assert torch.equal(net(x), y), "two eager forwards differ"


@pytest.mark.parametrize("name", list(R.CASES))
def test_whole_model_bf16(name):
    dev = _dev()
    net, g, meta = _net(name, "bf16", dev)
    x = torch.from_numpy(g["x"])
    res = net(x.to(dev)).cpu() - R.nearest(x, meta["cfg"]["upscale"])
    want = torch.from_numpy(g["res"])
    psnr, err = O.psnr_float(res, want), max_abs(res, want)
    dev_ = meta["bf16"]
    if dev_ is not None and math.isfinite(dev_["psnr"]) and math.isfinite(dev_["max_abs"]):
        bar_db, bar_abs = min(40.0, math.floor(dev_["psnr"])), 1.25 * dev_["max_abs"]
    else:
        bar_db, bar_abs = 40.0, 0.08
    print(f"srvgg_{name} bf16 residual: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})")
    assert psnr >= bar_db and err <= bar_abs, f"srvgg_{name} bf16 residual: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})"


def test_graph_replay_equals_eager_and_a_second_shape_recaptures():
    dev = _dev()
    net, g, _ = _net("b", "bf16", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    x2 = x[:1, :, :17, :20].contiguous()
    eager, eager2 = net(x), net(x2)
    net.use_graph = True
    try:
        assert torch.equal(net(x), eager) and torch.equal(net(x), eager)       # capture, then replay
        assert torch.equal(net(x2), eager2) and torch.equal(net(x2), eager2)   # another shape: captured again
        assert torch.equal(net(x), eager) and len(net._graphs) == 2
    finally:
        net.use_graph = False
    assert torch.equal(net(x), eager)


# ---- the frame paths: the bytes of the two-step composition -----------------------------------------------------------------
def _frame(seed, B, h, w, dev):
    return torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(dev)


def _planes_of(frame):
    from super_resolution_amd import ops
    b, h, w, _ = frame.shape
    x = torch.empty(b, 3, h, w, device=frame.device)
    ops.u8_to_planes(frame, x)
    return x


@pytest.mark.parametrize("name,S", [("b", 2), ("a", 4)], ids=["x2", "x4"])
def test_upscale_u8_and_to_u8_are_the_composition(name, S):
    """19 x 35, B = 2: upscale_u8(frame) == planes_to_u8(forward(u8_to_planes(frame))), through hat_shuffle_to_u8; upscale_to_u8 with a crop."""
    dev = _dev()
    from super_resolution_amd import ops
    net, _, _ = _net(name, "bf16", dev)
    eng = net.engine(dev)
    assert net.upscale == S
    frame = _frame(19 + S, 2, 19, 35, dev)
    x = _planes_of(frame)
    for bgr in (False, True):
        want = torch.empty(2, S * 19, S * 35, 3, dtype=torch.uint8, device=dev)
        xb = torch.empty_like(x)
        ops.u8_to_planes(frame, xb, bgr=bgr)
        ops.planes_to_u8(net(xb).contiguous(), want, bgr=bgr)
        before = (eng.u8_fused_calls, eng.u8_planes_calls)
        got = net.upscale_u8(frame, bgr=bgr)
        assert (eng.u8_fused_calls - before[0], eng.u8_planes_calls - before[1]) == (1, 0)
        assert torch.equal(got, want), f"x{S} bgr={bgr}: {int((got != want).sum())} of {want.numel()} bytes differ"
    crop = (S * 19 - 3, S * 35 - 5)
    want = torch.empty(2, S * 19, S * 35, 3, dtype=torch.uint8, device=dev)
    ops.planes_to_u8(net(x).contiguous(), want)
    assert torch.equal(net.upscale_to_u8(x, crop=crop), want[:, :crop[0], :crop[1]])
    assert torch.equal(net.upscale_to_u8(x), want)
    assert int(want.min()) == 0 and int(want.max()) == 255      # both clamps of the conversion are hit


YUV_CASES = [("nv12", "nv12", 8, 8), ("i420", "i420", 10, 10), ("uyvy", "uyvy", 8, 8), ("gray", "i444", 8, 8)]


@pytest.mark.parametrize("fmt,out_fmt,depth,out_depth", YUV_CASES, ids=[f"{a}_{d}_to_{b}" for a, b, d, _ in YUV_CASES])
def test_upscale_yuv_is_the_composition(fmt, out_fmt, depth, out_depth):
    """One case per kind of surface: semi-planar 8-bit, planar 10-bit, packed 4:2:2, grey in and 4:4:4 out; 20 x 36, B = 2, x2."""
    dev = _dev()
    from super_resolution_amd import ops, yuv
    net, _, _ = _net("b", "bf16", dev)
    eng, S, (h, w) = net.engine(dev), 2, (20, 36)
    p = _planes_of(_frame(77, 2, h, w, dev)).cpu().numpy()
    make = yuv.planes_to_packed if fmt in yuv.PACKED_FORMATS else yuv.planes_to_yuv
    fr = torch.from_numpy(make(p, fmt=fmt, out_depth=depth, **BT601))
    fr = (fr.view(torch.int16) if fr.dtype == torch.uint16 else fr).to(dev)
    fr = fr.view(torch.uint16) if depth > 8 else fr
    src, dst = ops.FrameSide(fmt, depth=depth), ops.FrameSide(out_fmt, depth=out_depth)
    assert src.size(fr.shape) == (h, w)
    x = torch.empty(2, 3, h, w, device=dev)
    src.to_planes(fr, x, yuv.csc(depth=depth, **BT601)[0], width=w)
    y = net(x).contiguous()
    want = dst.out(None, (2,) + dst.shape(S * h, S * w), dev)
    dst.from_planes(y, want, yuv.csc(depth=out_depth, **BT601)[1], width=S * w)
    before = (eng.yuv_fused_calls, eng.yuv_planes_calls)
    got = net.upscale_yuv(fr, fmt=fmt, out_fmt=out_fmt, depth=depth, out_depth=out_depth)
    ran = (eng.yuv_fused_calls - before[0], eng.yuv_planes_calls - before[1])
    raw = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
    assert got.shape == want.shape and torch.equal(raw(got), raw(want)), f"{fmt} -> {out_fmt}: differs from the composition"
    assert ran == ((0, 1) if dst.packed else (1, 0)), ran      # a packed output is written from planes, every other by hat_shuffle_to_yuv


def test_upscale_ensemble_is_the_mean_over_the_eight_transforms():
    dev = _dev()
    net, g, _ = _net("b", "bf16", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    ref = E.ensemble(net, x, 8)
    got = net.upscale_ensemble(x, 8)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and torch.equal(got, ref)
    assert torch.equal(net.upscale_ensemble(x, 1), net(x))


def test_any_frame_size_batches_and_refused_names():
    dev = _dev()
    net, _, _ = _net("b", "bf16", dev)
    assert tuple(net.upscale_u8(torch.zeros(1, 1, 3, dtype=torch.uint8, device=dev)).shape) == (1, 2, 2, 3)     # a 1 x 1 frame
    assert tuple(net(torch.zeros(3, 3, 1, 7, device=dev)).shape) == (3, 3, 2, 14)
    x = torch.zeros(1, 3, 8, 8, device=dev)
    for call in (lambda: net.forward_ensemble(x), lambda: net.forward_to_u8(x), lambda: net.forward_yuv420(x), lambda: net.forward_bands(x, 2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(RuntimeError, match=r"\(B,3,h,w\)"):
        net(torch.zeros(1, 4, 8, 8, device=dev))


# ---- the harness on the fixture option file ---------------------------------------------------------------------------------
def _fixture_opt(tmp_path, datasets, val=None, **extra):
    import yaml
    with open(os.path.join(R.GOLDEN, "srvgg_x4_toy.yml")) as f:
        opt = yaml.safe_load(f)
    cfg, sd, _, _ = R.load_case("a")
    assert {k: v for k, v in opt["network_g"].items() if k != "type"} == cfg
    torch.save({"params": sd}, tmp_path / "net.pth")
    opt["datasets"] = datasets
    opt["path"] = dict(opt["path"], pretrain_network_g=str(tmp_path / "net.pth"), visualization=str(tmp_path / "vis"))
    opt["val"] = dict(opt["val"], **(val or {}))
    opt.update(extra)
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    return str(tmp_path / "opt.yml")


def test_harness_float_u8_and_metrics_on_device_agree(tmp_path):
    """`python -m super_resolution_amd.test` on the fixture option file (SRModel, SRVGGNetCompact x4, no window_size) with a two-image
    synthetic dataset: --u8 / --metrics-on-device write the PNGs the float run writes, byte for byte, and the device scores are the
    float run's host scores within 1e-8 dB / 1e-10 SSIM, as for ESC (tests/test_gpu_esc_frames.py); the tiled run, the self-ensemble
    and --lq-on-device run too."""
    _dev()
    from super_resolution_amd import data as D, metrics as M, synth, test as T
    for i, (h, w) in enumerate([(21, 26), (19, 35)]):
        gt = synth.synth_input(40 + i, (1, 3, 4 * h, 4 * w))
        D.write_image(M.tensor2img(gt), str(tmp_path / "gt" / f"im{i}.png"))
        D.write_image(M.tensor2img(F.avg_pool2d(gt, 4)), str(tmp_path / "lq" / f"im{i}.png"))
    ds = {"test_1": {"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"), "dataroot_lq": str(tmp_path / "lq"),
                     "io_backend": {"type": "disk"}}}
    res = {}
    for mode, flags, extra in (("float", [], {}), ("u8", ["--u8", "--metrics-on-device"], {}), ("tile", [], {"tile": {"tile_size": 16, "tile_pad": 4}}),
                               ("tile_u8", ["--u8"], {"tile": {"tile_size": 16, "tile_pad": 4}}), ("ens", ["--self-ensemble", "4"], {}),
                               ("ens_u8", ["--self-ensemble", "4", "--u8"], {}), ("lq_dev", ["--lq-on-device", "--metrics-on-device"], {})):
        (tmp_path / mode).mkdir()
        res[mode] = T.main(["-opt", _fixture_opt(tmp_path / mode, ds, **extra)] + flags)["Toy"]
    png = lambda mode, i: D.read_image(str(tmp_path / mode / "vis" / "Toy" / f"im{i}_SRVGG_toy_x4.png"))
    for i, (h, w) in enumerate([(21, 26), (19, 35)]):
        assert tuple(png("float", i).shape) == (3, 4 * h, 4 * w)
        for a, b in (("float", "u8"), ("tile", "tile_u8"), ("ens", "ens_u8")):
            assert torch.equal(png(a, i), png(b, i)), f"im{i}: the {b} run's PNG differs from the {a} run's"
        assert not torch.equal(png("float", i), png("ens", i)) and tuple(png("lq_dev", i).shape) == (3, 4 * h, 4 * w)
        fa, fb = res["float"]["images"][i], res["u8"]["images"][i]
        assert abs(fa["psnr"] - fb["psnr"]) <= 1e-8 and abs(fa["ssim"] - fb["ssim"]) <= 1e-10, (fa, fb)


def test_video_tool_on_the_fixture_option_file(tmp_path):
    """A 2-frame 20 x 24 Y4M through `python -m super_resolution_amd.video`: a Y4M of 80 x 96 whose frames are upscale_frames'."""
    _dev()
    from super_resolution_amd import frames, video, y4m
    from super_resolution_amd.models import HATModel
    from super_resolution_amd.test import parse_options
    opt = _fixture_opt(tmp_path, {})
    rng = np.random.default_rng(5)
    src = [rng.integers(16, 236, (30, 24), dtype=np.uint8) for _ in range(2)]
    with y4m.Writer(str(tmp_path / "in.y4m"), dict(W=24, H=20, F="25:1", C="420jpeg"), chroma=True) as wr:
        for f in src:
            wr.write(f)
    info = video.main(["-opt", opt, "-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.y4m")])
    assert info["frames"] == 2 and info["out"] == (96, 80)
    model = HATModel(parse_options(opt), device="cuda:0")
    want = list(frames.upscale_frames(model.get_bare_model(model.net_g), src, pixfmt="i420"))
    with y4m.Reader(str(tmp_path / "out.y4m"), chroma=True) as rd:
        got = list(rd)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))
