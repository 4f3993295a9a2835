"""ESCReal on the device: hat_escreal_skip, hat_dysample and the slope-0.2 LeakyReLU of hat_conv against fp64 restatements of the same
operation on the kernels' own inputs (tests/escreal_ref.py), the whole model against the reference's goldens
(tests/golden/escreal_*.npz, gen_golden_escreal.py), eager against graph replay, and a reference-style option file through
`python -m super_resolution_amd.test`.

Bars: fp32 1e-4 max-abs (the project's fp32 bar).  bf16 kernels: helpers.check's bar.  bf16 whole model: where the reference's own
bf16 run is finite (the default head) its PSNR rounded down to a whole dB and capped at 40, and its max-abs x 1.25, as for ESC;
where it is not (DySample: the reference's bf16 grid_sample returns NaN / 1e31 on the CPU, recorded as null) the project-wide
bf16 bar, >= 40 dB and max-abs <= 0.08."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import escreal_ref as R
from helpers import check, max_abs, q, rnd
from oracle import hat_oracle as O
from super_resolution_amd import synth

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rows(x_bchw, ld, tdt, dev, fill=7.0):
    _, c, h, w = x_bchw.shape
    out = torch.full((1, h * w, ld), fill, dtype=tdt, device=dev)
    out[:, :, :c] = x_bchw[0].reshape(c, h * w).t().to(dev).to(tdt)
    return out


def _maps(rows, c, h, w):
    return rows[0, :, :c].float().cpu().t().reshape(1, c, h, w)


# ---- hat_escreal_skip -------------------------------------------------------------------------------------------------------
def _skip_sd():
    return {"skip.0.weight": rnd("s0w", (128, 3, 1, 1)), "skip.0.bias": rnd("s0b", (128,)),
            "skip.1.weight": rnd("s1w", (128, 1, 7, 7), std=1 / 7), "skip.1.bias": rnd("s1b", (128,)),
            "skip.3.weight": rnd("s3w", (64, 128, 1, 1), std=128 ** -0.5), "skip.3.bias": rnd("s3b", (64,))}


def _run_skip(sd, x, dtype, with_r, dev):
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    _, _, h, w = x.shape
    ps = ops.pack_escreal_skip(sd, "skip", dt, dev)
    r = rnd(f"skr{h}x{w}", (1, 64, h, w))
    out = torch.full((1, h * w, 72), 7.0, device=dev)
    ops.escreal_skip(ps, x.to(dev), out, B=1, H=h, W=w, dtype=dt, r=_rows(r, 68, torch.float32, dev) if with_r else None, ldr=68, ldo=72)
    torch.cuda.synchronize()
    assert float((out[0, :, 64:] - 7.0).abs().max()) == 0.0, "pad channels written"
    return _maps(out, 64, h, w), (r.double() if with_r else 0.0)


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "r"])
@pytest.mark.parametrize("hw", [(4, 4), (5, 7)])   # 4x4: the smallest legal frame, every tap of every pixel but the centre column / row is reflected
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_skip_matches_fp64_on_small_frames(dtype, hw, with_r):
    dev = _dev()
    sd, x = _skip_sd(), q(rnd(f"skx{hw}", (1, 3) + hw), dtype)
    got, r = _run_skip(sd, x, dtype, with_r, dev)
    check(got, R.skip_branch(x.double(), R.d64(sd)) + r, dtype, f"hat_escreal_skip {hw}", f32_tol=1e-4)


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "r"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_skip_matches_the_reference_rows_on_33x40(dtype, with_r):
    """Case a's weights and frame: 21 tiles of 64 pixels, the last one ragged; the reference's own skip(x) at the tap pixels."""
    dev = _dev()
    _, sd, g, _ = R.load_case("a")
    got, r = _run_skip(sd, torch.from_numpy(g["x"]), dtype, with_r, dev)
    px = torch.from_numpy(g["tap_pixels"])
    want = torch.from_numpy(g["skip"]).double() + (R.rows_at(r, px) if with_r else 0.0)
    check(R.rows_at(got, px), want, dtype, "hat_escreal_skip 33x40 vs the reference", f32_tol=1e-4)
    full = R.skip_branch(torch.from_numpy(g["x"]).double(), R.d64(sd)) + r
    check(got, full, dtype, "hat_escreal_skip 33x40", f32_tol=1e-4)


def test_skip_refuses_bad_arguments_before_any_launch():
    dev = _dev()
    from super_resolution_amd import _lib, ops
    lib = _lib.load()
    ps = ops.pack_escreal_skip(_skip_sd(), "skip", ops.HAT_F32, dev)
    x = torch.zeros(1, 3, 8, 8, device=dev)
    out = torch.full((1, 64, 64 + 4), 7.0, device=dev)
    r = torch.zeros(1, 64, 64, device=dev)
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(x=P(x), w1=P(ps.w1), b1=P(ps.b1), w3=P(ps.w3), b3=P(ps.b3), r=P(r), out=P(out), B=1, H=8, W=8, ldr=64, ldo=68, dtype=ops.HAT_F32)
    order = ("x", "w1", "b1", "w3", "b3", "r", "out", "B", "H", "W", "ldr", "ldo", "dtype")
    call = lambda **kw: lib.hat_escreal_skip(*[dict(good, **kw)[k] for k in order], torch.cuda.current_stream().cuda_stream)
    bad = [dict(x=None), dict(w1=None), dict(b1=None), dict(w3=None), dict(b3=None), dict(out=None),       # null pointers
           dict(out=P(out) + 4), dict(w1=P(ps.w1) + 8), dict(b3=P(ps.b3) + 4), dict(r=P(r) + 4), dict(x=P(x) + 2),   # misaligned
           dict(ldo=62), dict(ldo=66), dict(ldr=60), dict(ldr=66),                                                   # leading dimensions
           dict(H=3), dict(W=3), dict(H=0), dict(B=0), dict(B=65536), dict(dtype=7)]
    for kw in bad:
        assert call(**kw) == -1, f"{kw}: expected HAT_EINVAL"
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0, "a refused call launched"
    assert call() == 0 and call(r=None) == 0
    torch.cuda.synchronize()
    assert float((out[0, :, :64] - 7.0).abs().min()) > 0.0 and float((out[0, :, 64:] - 7.0).abs().max()) == 0.0


# ---- hat_dysample -----------------------------------------------------------------------------------------------------------
def _run_dysample(feat, sd, s, dev, offset_scale=1.0):
    """hat_dysample alone: the rows [offset | scope | proj] are made on the host in fp64 and uploaded as fp32."""
    from super_resolution_amd import ops, packing
    sd = R.d64(sd)
    _, _, h, w = feat.shape
    wd, bd = packing.dysample_fold(sd["to_img.offset.weight"], sd["to_img.offset.bias"], sd["to_img.scope.weight"], sd["to_img.end_conv.weight"])
    rows = F.conv2d(feat.double(), wd[:, :, None, None], bd)
    rows[:, :8 * s * s] *= offset_scale
    ld = wd.shape[0] + 4
    y = torch.zeros(1, 3, s * h, s * w, device=dev)
    ops.dysample(_rows(rows, ld, torch.float32, dev), sd["to_img.init_pos"].float().reshape(-1).to(dev), sd["to_img.end_conv.bias"].float().to(dev),
                 y, B=1, H=h, W=w, s=s, ld=ld)
    torch.cuda.synchronize()
    return y.cpu(), R.head_dysample(feat.double(), sd, s, offset_scale=offset_scale)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_dysample_matches_fp64_on_the_reference_feat_rows(s):
    """The reference's to_img input at the 160 tap pixels laid out as a 10 x 16 map, offsets at std 0.3: samples on every side of
    the frame are clamped, others lie several pixels from their own."""
    dev = _dev()
    _, sd, g, _ = R.load_case({2: "e", 3: "d", 4: "c"}[s])
    feat = torch.from_numpy(g["feat"]).t().reshape(1, 64, 10, 16)
    px, py = R.dys_positions(feat.double(), R.d64(sd), s)
    assert (px < 0).any() and (px > 15).any() and (py < 0).any() and (py > 9).any()
    got, want = _run_dysample(feat, sd, s, dev)
    check(got, want, "f32", f"hat_dysample x{s}", f32_tol=1e-4)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_dysample_with_every_sample_clamped_and_with_zero_offsets(s):
    dev = _dev()
    _, sd, _, _ = R.load_case({2: "e", 3: "d", 4: "c"}[s])
    feat = rnd(f"dysf{s}", (1, 64, 9, 13))
    px, py = R.dys_positions(feat.double(), R.d64(sd), s, offset_scale=1e5)
    assert bool((((px < 0) | (px > 12)) | ((py < 0) | (py > 8))).all()), "a sample is not clamped"
    got, want = _run_dysample(feat, sd, s, dev, offset_scale=1e5)
    check(got, want, "f32", f"hat_dysample x{s}, clamped", f32_tol=1e-4)
    got, want = _run_dysample(feat, sd, s, dev, offset_scale=0.0)   # init_pos alone: a fixed bilinear x s upsampling per group
    check(got, want, "f32", f"hat_dysample x{s}, zero offsets", f32_tol=1e-4)


def test_dysample_refusals():
    dev = _dev()
    from super_resolution_amd import ops
    z, y = torch.zeros(1, 35, 80, device=dev), torch.zeros(1, 3, 10, 14, device=dev)
    ip, b = torch.zeros(32, device=dev), torch.zeros(3, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.dysample(z, ip, b, y, B=1, H=5, W=7, s=2, ld=72)      # 16 s^2 + 12 = 76 values per pixel
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.dysample(z, ip, b, y, B=1, H=5, W=7, s=5, ld=80)


# ---- HAT_ACT_LRELU02 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lrelu02_through_hat_conv_pixshuf(dtype):
    """nearest x2 + conv + LeakyReLU(0.2) as the folded conv with HAT_O_PIXSHUF_T on 21x19: no multiple of a conv tile."""
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    h, w = 21, 19
    wt, b, x = rnd("l2w", (64, 64, 3, 3), std=1 / 24), rnd("l2b", (64,), std=0.1), q(rnd("l2x", (1, 64, h, w)), dtype)
    pw = ops.pack_nearest_conv(wt, b, dt, dev)
    out = torch.full((1, 4 * h * w, 72), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.conv(pw, _rows(x, 64, ops.TORCH_DTYPE[dt], dev), out, B=1, H=h, W=w, dtype=dt, ldx=64, ldo=72, out_mode=ops.O_PIXSHUF_T, ps_r=2,
             act=ops.ACT_LRELU02)
    torch.cuda.synchronize()
    want = R.lrelu(F.conv2d(R.nearest2(x.double()), wt.double(), b.double(), padding=1))
    assert float(want.min()) < -0.5   # the negative side is there, and slope 0.01 would be far away
    check(_maps(out, 64, 2 * h, 2 * w), want, dtype, "hat_conv + LRELU02 + pixel shuffle", f32_tol=1e-4)
    assert float((out[0, :, 64:].float() - 7.0).abs().max()) == 0.0, "pad channels written"


def test_lrelu02_is_declined_where_it_is_not_built():
    dev = _dev()
    from super_resolution_amd import ops
    pw = ops.pack_linear_weight(rnd("l2lw", (64, 64)), None, ops.HAT_F32, dev)
    x, out = torch.zeros(1, 35, 64, device=dev), torch.zeros(1, 35, 64, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.linear(pw, x, out, B=1, H=5, W=7, dtype=ops.HAT_F32, ldx=64, ldo=64, act=ops.ACT_LRELU02)
    pc = ops.pack_conv_weight(rnd("l2cw", (64, 64, 3, 3)), None, ops.HAT_F32, dev)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.conv(pc, x, out, B=1, H=5, W=7, dtype=ops.HAT_F32, ldx=64, ldo=64, act=4)


# ---- whole model ------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name, dtype, dev):
    from super_resolution_amd.registry import build_network
    if (name, dtype) not in _NETS:
        cfg, sd, g, meta = R.load_case(name)
        net = build_network(dict(cfg, type="ESCReal", attn_type="Naive", compute_dtype=dtype)).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[(name, dtype)] = (net.to(dev), g, meta)
    return _NETS[(name, dtype)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_whole_model_fp32_matches_reference(name):
    dev = _dev()
    net, g, meta = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    y = net(x)
    assert list(y.shape) == meta["out"]
    err = max_abs(y.cpu(), g["y"])
    print(f"escreal_{name} y: max-abs {err:.3e}")
    assert err <= 1e-4, f"escreal_{name}: max-abs {err:.3e}"
    assert torch.equal(net(x), y), "two eager forwards differ"


@pytest.mark.parametrize("name", list(R.CASES))
def test_whole_model_bf16(name):
    dev = _dev()
    net, g, meta = _net(name, "bf16", dev)
    y = net(torch.from_numpy(g["x"]).to(dev)).cpu()
    psnr, err = O.psnr_float(y, torch.from_numpy(g["y"])), max_abs(y, g["y"])
    if meta["bf16"] is not None:
        bar_db, bar_abs = min(40.0, math.floor(meta["bf16"]["psnr"])), 1.25 * meta["bf16"]["max_abs"]
    else:
        bar_db, bar_abs = 40.0, 0.08
    print(f"escreal_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})")
    assert psnr >= bar_db and err <= bar_abs, f"escreal_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})"


@pytest.mark.parametrize("name", ["a", "c"])
def test_graph_replay_equals_eager(name):
    dev = _dev()
    net, g, _ = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    eager = net(x)
    assert torch.equal(net(x), eager)
    net.use_graph = True
    try:
        assert torch.equal(net(x), eager) and torch.equal(net(x), eager)   # capture, then replay
    finally:
        net.use_graph = False
    assert torch.equal(net(x), eager)


def test_refused_paths_and_frames():
    dev = _dev()
    net, _, _ = _net("a", "fp32", dev)
    x = torch.zeros(1, 3, 40, 40, device=dev)
    for call in (lambda: net.forward_ensemble(x), lambda: net.forward_to_u8(x), lambda: net.forward_yuv420(x), lambda: net.forward_bands(x, 2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(RuntimeError, match="one frame"):
        net(torch.zeros(2, 3, 40, 40, device=dev))
    with pytest.raises(RuntimeError, match="reflect-padded"):
        net(torch.zeros(1, 3, 3, 40, device=dev))
    with pytest.raises(RuntimeError, match="at least 4"):
        net.engine(dev)._check_frame(3, 40)


def test_reference_style_yaml_through_the_test_entry(tmp_path):
    """An option file as the reference's ESC_Real_X4 (model_type ESRModel, network_g.type ESCReal, a GT-less SingleImageDataset)
    through `python -m super_resolution_amd.test`: the saved images are tensor2img of the fp32 restatement's output on the host,
    up to one grey level where a value sits on a rounding boundary."""
    dev = _dev()
    import yaml
    from super_resolution_amd import data as D, metrics as M, test as T
    cfg, sd, _, _ = R.load_case("a")
    torch.save({"params": sd}, tmp_path / "net.pth")
    sizes = [(40, 45), (36, 50)]
    for i, (h, w) in enumerate(sizes):
        D.write_image(M.tensor2img(synth.synth_input(30 + i, (1, 3, h, w))), str(tmp_path / "lq" / f"im{i}.png"))
    opt = {"name": "ESC_Real_toy_X4", "model_type": "ESRModel", "scale": 4, "num_gpu": 1,
           "datasets": {"test_1": {"name": "Toy", "type": "SingleImageDataset", "dataroot_lq": str(tmp_path / "lq"), "io_backend": {"type": "disk"}}},
           "network_g": dict(cfg, type="ESCReal", attn_type="Naive", compute_dtype="fp32"),
           "path": {"pretrain_network_g": str(tmp_path / "net.pth"), "strict_load_g": True, "param_key_g": "params",
                    "visualization": str(tmp_path / "vis")},
           "val": {"save_img": True, "suffix": None}}
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    res = T.main(["-opt", str(tmp_path / "opt.yml")])
    assert len(res["Toy"]["images"]) == 2
    for i, (h, w) in enumerate(sizes):
        lq = D.read_image(str(tmp_path / "lq" / f"im{i}.png")).unsqueeze(0)
        xp = F.pad(lq, (0, (-w) % 32, 0, (-h) % 32), "reflect")
        want = M.tensor2img(R.forward(sd, cfg, xp)[:, :, :4 * h, :4 * w]).astype(np.int32)
        got = M.tensor2img(D.read_image(str(tmp_path / "vis" / "Toy" / f"im{i}_ESC_Real_toy_X4.png")).unsqueeze(0)).astype(np.int32)
        assert got.shape == want.shape == (4 * h, 4 * w, 3)
        diff = np.abs(got - want)
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (int(diff.max()), float((diff > 0).mean()))
