"""ESCRealM on the device: hat_unshuffle_pad, hat_escrealm_skip, hat_shuffle_planes, the slope-0.01 LeakyReLU and the x3 nearest fold
through hat_conv, hat_dysample behind a 48-channel map — each against the fp64 restatement of the same operation on the kernel's own
inputs (tests/escrealm_ref.py) — the whole model against the reference's goldens (tests/golden/escrealm_*.npz,
gen_golden_escrealm.py), eager against graph replay, tile_parallel, and an option file through `python -m super_resolution_amd.test`.

Bars: fp32 1e-4 max-abs (the project's fp32 bar).  bf16 kernels: helpers.check's bar.  bf16 whole model: where the reference's own
bf16 run is finite its PSNR rounded down to a whole dB and capped at 40, and its max-abs x 1.25, as for ESC; where it is not (case f,
DySample: the reference's bf16 grid_sample is not finite on the CPU, recorded as null) the project-wide bf16 bar, >= 40 dB and
max-abs <= 0.08, as for ESCReal."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import escrealm_ref as R
from helpers import check, max_abs, q, rnd
from oracle import hat_oracle as O
from super_resolution_amd import synth
from test_gpu_escreal import _dev, _maps, _rows

pytestmark = pytest.mark.gpu


# ---- hat_unshuffle_pad ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (66, 83), (8, 12)])   # both pads live; pads of 2 and 1 at f=4; already a multiple of f
@pytest.mark.parametrize("f", [2, 4])
def test_unshuffle_pad_is_exact(f, hw):
    dev = _dev()
    from super_resolution_amd import ops
    h, w = hw
    x = rnd(f"ux{f}{hw}", (1, 3, h, w))
    want = R.unshuffle_pad(x, f)
    cin, (Hb, Wb) = 3 * f * f, want.shape[-2:]
    assert torch.equal(want, F.pixel_unshuffle(F.pad(x, (0, Wb * f - w, 0, Hb * f - h), "reflect"), f)), "the restatement"
    rows = torch.full((1, Hb * Wb, cin + 4), 7.0, device=dev)
    ops.unshuffle_pad(x.to(dev), rows, B=1, h=h, w=w, f=f, ld=cin + 4)
    torch.cuda.synchronize()
    assert torch.equal(_maps(rows, cin, Hb, Wb), want)
    assert float((rows[0, :, cin:] - 7.0).abs().max()) == 0.0, "pad channels written"


# ---- hat_escrealm_skip ------------------------------------------------------------------------------------------------------
def _skip_sd(cin):
    return {"skip.1.weight": rnd(f"m1w{cin}", (128, cin, 1, 1), std=cin ** -0.5), "skip.1.bias": rnd("m1b", (128,)),
            "skip.2.weight": rnd("m2w", (128, 1, 7, 7), std=1 / 7), "skip.2.bias": rnd("m2b", (128,)),
            "skip.4.weight": rnd("m4w", (64, 128, 1, 1), std=128 ** -0.5), "skip.4.bias": rnd("m4b", (64,))}


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "r"])
@pytest.mark.parametrize("hw", [(10, 16), (4, 4)])   # 10x16: four 8x8 tiles, two ragged; 4x4: the reflection reaches the far border
@pytest.mark.parametrize("cin", [12, 48])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_wide_skip_matches_fp64(dtype, cin, hw, with_r):
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    h, w = hw
    sd, x = _skip_sd(cin), rnd(f"mx{cin}{hw}", (1, cin, h, w))
    ps = ops.pack_escrealm_skip(sd, "skip", dt, dev)
    r = rnd(f"mr{hw}", (1, 64, h, w))
    out = torch.full((1, h * w, 72), 7.0, device=dev)
    ops.escrealm_skip(ps, _rows(x, cin + 4, torch.float32, dev), out, B=1, H=h, W=w, dtype=dt, ldx=cin + 4,
                      r=_rows(r, 68, torch.float32, dev) if with_r else None, ldr=68, ldo=72)
    torch.cuda.synchronize()
    assert float((out[0, :, 64:] - 7.0).abs().max()) == 0.0, "pad channels written"
    want = R.skip_branch(x.double(), R.d64(sd), first=1) + (r.double() if with_r else 0.0)
    check(_maps(out, 64, h, w), want, dtype, f"hat_escrealm_skip {cin} {hw}", f32_tol=1e-4)


@pytest.mark.parametrize("name", ["a", "b"])
def test_wide_skip_matches_the_reference_rows(name):
    """Case a's (12 channels, 34x41) and b's (48 channels, 17x21) weights and frame: the reference's own skip(x) at the tap pixels."""
    dev = _dev()
    from super_resolution_amd import ops
    cfg, sd, g, meta = R.load_case(name)
    f, _ = R.stem_of(cfg)
    xu = R.unshuffle_pad(torch.from_numpy(g["x"]), f)
    (H, W), cin = meta["body"], 3 * f * f
    ps = ops.pack_escrealm_skip(sd, "skip", ops.HAT_F32, dev)
    out = torch.zeros(1, H * W, 64, device=dev)
    ops.escrealm_skip(ps, _rows(xu, cin, torch.float32, dev), out, B=1, H=H, W=W, dtype=ops.HAT_F32, ldx=cin)
    torch.cuda.synchronize()
    check(R.rows_at(_maps(out, 64, H, W), torch.from_numpy(g["tap_pixels"])), torch.from_numpy(g["skip"]).double(), "f32",
          f"hat_escrealm_skip case {name} vs the reference", f32_tol=1e-4)


def test_new_entries_refuse_bad_arguments_before_any_launch():
    dev = _dev()
    from super_resolution_amd import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ps = ops.pack_escrealm_skip(_skip_sd(12), "skip", ops.HAT_F32, dev)
    x, out = torch.zeros(1, 64, 12, device=dev), torch.full((1, 64, 68), 7.0, device=dev)
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(x=P(x), w0=P(ps.w0), b0=P(ps.b0), dw=P(ps.dw), bdw=P(ps.bdw), w3=P(ps.w3), b3=P(ps.b3), r=None, out=P(out), B=1, H=8, W=8, cin=12,
                ldx=12, ldr=64, ldo=68, dtype=ops.HAT_F32)
    call = lambda **kw: lib.hat_escrealm_skip(*dict(good, **kw).values(), st)
    for kw in [dict(x=None), dict(w0=None), dict(dw=None), dict(w3=None), dict(out=None), dict(x=P(x) + 4), dict(out=P(out) + 4), dict(ldx=8),
               dict(ldx=14), dict(ldo=62), dict(H=3), dict(W=3), dict(B=0), dict(B=65536), dict(dtype=7), dict(r=P(out) + 4)]:
        assert call(**kw) == -1, f"{kw}: expected HAT_EINVAL"
    assert call(cin=16, ldx=16) == -3 and call(cin=3) == -3
    img, rows = torch.zeros(1, 3, 5, 7, device=dev), torch.full((1, 12, 16), 7.0, device=dev)
    assert lib.hat_unshuffle_pad(None, P(rows), 1, 5, 7, 2, 12, st) == -1 and lib.hat_unshuffle_pad(P(img), P(rows), 1, 5, 7, 2, 8, st) == -1
    assert lib.hat_unshuffle_pad(P(img), P(rows), 1, 5, 7, 3, 27, st) == -3 and lib.hat_unshuffle_pad(P(img), P(rows), 1, 1, 7, 4, 48, st) == -1
    assert lib.hat_shuffle_planes(None, P(rows), 1, 3, 4, 2, 12, st) == -1 and lib.hat_shuffle_planes(P(img), P(rows), 1, 3, 4, 2, 8, st) == -1
    assert lib.hat_shuffle_planes(P(img), P(rows), 1, 3, 4, 9, 243, st) == -1
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0 and float((rows - 7.0).abs().max()) == 0.0, "a refused call launched"
    assert call() == 0


# ---- hat_shuffle_planes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_shuffle_planes_is_exact(s):
    dev = _dev()
    from super_resolution_amd import ops
    h, w, c = 9, 13, 3 * s * s
    t = rnd(f"sp{s}", (1, c, h, w))
    y = torch.zeros(1, 3, s * h, s * w, device=dev)
    ops.shuffle_planes(_rows(t, c + 4, torch.float32, dev), y, B=1, H=h, W=w, s=s, ld=c + 4)
    torch.cuda.synchronize()
    assert torch.equal(R.pixel_shuffle(t, s), F.pixel_shuffle(t, s)) and torch.equal(y.cpu(), F.pixel_shuffle(t, s))


# ---- hat_conv: LeakyReLU 0.01, the x3 nearest fold, PixelShuffle(3) ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lrelu001_through_hat_conv(dtype):
    """to_img.0 of the pixelshuffle / dysample heads: 3x3 64 -> 48 + nn.LeakyReLU() on 21x19."""
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    h, w = 21, 19
    wt, b, x = rnd("l1w", (48, 64, 3, 3), std=1 / 24), rnd("l1b", (48,), std=0.1), q(rnd("l1x", (1, 64, h, w)), dtype)
    out = torch.full((1, h * w, 56), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.conv(ops.pack_conv_weight(wt, b, dt, dev), _rows(x, 64, ops.TORCH_DTYPE[dt], dev), out, B=1, H=h, W=w, dtype=dt, ldx=64, ldo=56, act=ops.ACT_LRELU)
    torch.cuda.synchronize()
    pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    assert float(pre.min()) < -0.5   # the negative side is there, and slope 0.2 would be far away
    check(_maps(out, 48, h, w), R.lrelu(pre, 0.01), dtype, "hat_conv + LRELU 0.01", f32_tol=1e-4)
    assert float((out[0, :, 48:].float() - 7.0).abs().max()) == 0.0, "pad channels written"


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_conv_nearest_fold_against_interpolate(dtype, r):
    """conv -> F.interpolate(nearest, r) -> LeakyReLU(0.2) as the folded conv with HAT_O_PIXSHUF_T on 21x19."""
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    h, w = 21, 19
    wt, b, x = rnd("n3w", (64, 64, 3, 3), std=1 / 24), rnd("n3b", (64,), std=0.1), q(rnd("n3x", (1, 64, h, w)), dtype)
    out = torch.full((1, r * r * h * w, 72), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.conv(ops.pack_conv_nearest(wt, b, r, dt, dev), _rows(x, 64, ops.TORCH_DTYPE[dt], dev), out, B=1, H=h, W=w, dtype=dt, ldx=64, ldo=72,
             out_mode=ops.O_PIXSHUF_T, ps_r=r, act=ops.ACT_LRELU02)
    torch.cuda.synchronize()
    want = R.lrelu(F.interpolate(F.conv2d(x.double(), wt.double(), b.double(), padding=1), scale_factor=r, mode="nearest"))
    check(_maps(out, 64, r * h, r * w), want, dtype, f"conv + nearest x{r} + LRELU02", f32_tol=1e-4)
    assert float((out[0, :, 64:].float() - 7.0).abs().max()) == 0.0, "pad channels written"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pixelshuffle3_at_48_channels(dtype):
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    h, w = 11, 19
    wt, b, x = rnd("p3w", (432, 48, 3, 3), std=1 / 21), rnd("p3b", (432,), std=0.1), q(rnd("p3x", (1, 48, h, w)), dtype)
    out = torch.full((1, 9 * h * w, 56), 7.0, dtype=ops.TORCH_DTYPE[dt], device=dev)
    ops.conv(ops.pack_pixshuf_conv(wt, b, 3, dt, dev), _rows(x, 48, ops.TORCH_DTYPE[dt], dev), out, B=1, H=h, W=w, dtype=dt, ldx=48, ldo=56,
             out_mode=ops.O_PIXSHUF_T, ps_r=3)
    torch.cuda.synchronize()
    check(_maps(out, 48, 3 * h, 3 * w), F.pixel_shuffle(F.conv2d(x.double(), wt.double(), b.double(), padding=1), 3), dtype, "conv 48 -> 432 + PixelShuffle(3)",
          f32_tol=1e-4)


# ---- hat_dysample behind 48 channels -----------------------------------------------------------------------------------------
def test_dysample_at_48_channels():
    """Case f's DySample (x4, 48 channels in 4 groups of 12) on a seeded 9x13 map: the pointwise fold through the engine's own
    launch, then hat_dysample, against the restatement; samples clamp on every side."""
    dev = _dev()
    from super_resolution_amd import ops
    _, sd, _, _ = R.load_case("f")
    p = R.dys_prefix(sd)
    dsd = {"to_img" + k[len(p):]: v for k, v in R.d64(sd).items() if k.startswith(p + ".")}
    h, w, s = 9, 13, 4
    feat = rnd("dys48", (1, 48, h, w))
    px, py = R.escreal_ref.dys_positions(feat.double(), dsd, s)
    assert (px < 0).any() and (px > w - 1).any() and (py < 0).any() and (py > h - 1).any()
    wd, bd = ops.dysample_fold(dsd["to_img.offset.weight"], dsd["to_img.offset.bias"], dsd["to_img.scope.weight"], dsd["to_img.end_conv.weight"])
    rows = F.conv2d(feat.double(), wd[:, :, None, None], bd)
    ld = wd.shape[0]
    y = torch.zeros(1, 3, s * h, s * w, device=dev)
    ops.dysample(_rows(rows, ld, torch.float32, dev), dsd["to_img.init_pos"].float().reshape(-1).to(dev), dsd["to_img.end_conv.bias"].float().to(dev), y,
                 B=1, H=h, W=w, s=s, ld=ld)
    torch.cuda.synchronize()
    check(y.cpu(), R.escreal_ref.head_dysample(feat.double(), dsd, s), "f32", "hat_dysample x4, 48 channels", f32_tol=1e-4)


# ---- whole model ------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name, dtype, dev):
    from super_resolution_amd.registry import build_network
    if (name, dtype) not in _NETS:
        cfg, sd, g, meta = R.load_case(name)
        net = build_network(dict(cfg, type="ESCRealM", attn_type="Naive", compute_dtype=dtype)).eval()
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
    print(f"escrealm_{name} y: max-abs {err:.3e}")
    assert err <= 1e-4, f"escrealm_{name}: max-abs {err:.3e}"
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
    print(f"escrealm_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})")
    assert psnr >= bar_db and err <= bar_abs, f"escrealm_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})"


@pytest.mark.parametrize("name", ["a", "d"])
def test_graph_replay_equals_eager_on_a_second_input(name):
    dev = _dev()
    net, g, _ = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    x2 = synth.synth_input(77, tuple(x.shape)).to(dev)
    eager, eager2 = net(x), net(x2)
    net.use_graph = True
    try:
        assert torch.equal(net(x), eager) and torch.equal(net(x2), eager2)   # capture, then replay on another input
    finally:
        net.use_graph = False
    assert torch.equal(net(x2), eager2)


def test_tile_parallel_on_one_rank():
    """tile_parallel's tiles (32 with overlap 8) through `forward` on one rank: every padded tile is a frame of its own (40x40,
    unshuffled to 20x20), its x2 core stitched; against the fp64 restatement run over the same tiles."""
    dev = _dev()
    from super_resolution_amd import tile_parallel as tp
    net, g, _ = _net("a", "fp32", dev)
    cfg, sd, _, _ = R.load_case("a")
    x = torch.from_numpy(g["x"])[:, :, :64, :64].contiguous()
    tiles = tp.reference_tiles(64, 64, 32, 8)
    y = tp.tile_forward(x.to(dev), net, net.upscale, tiles)
    sd64 = R.d64(sd)
    want = tp.tile_forward(x.double(), lambda t: R.forward(sd64, cfg, t), 2, tiles)
    assert tuple(y.shape) == (1, 3, 128, 128)
    assert max_abs(y.cpu(), want) <= 1e-4


def test_refused_paths_and_frames():
    dev = _dev()
    net, _, _ = _net("a", "fp32", dev)
    x = torch.zeros(1, 3, 40, 40, device=dev)
    for call in (lambda: net.forward_ensemble(x), lambda: net.forward_to_u8(x), lambda: net.forward_yuv420(x), lambda: net.forward_bands(x, 2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(RuntimeError, match="one frame"):
        net(torch.zeros(2, 3, 40, 40, device=dev))
    with pytest.raises(RuntimeError, match="at least 4|reflect-padded"):
        net(torch.zeros(1, 3, 6, 40, device=dev))   # unshuffled to 3x20
    with pytest.raises(RuntimeError, match="at least 4"):
        net.engine(dev)._check_frame(3, 40)


def test_option_file_through_the_test_entry(tmp_path):
    """An ESRModel option file with network_g.type ESCRealM (x2, the unshuffled stem) through `python -m super_resolution_amd.test`:
    the saved images are tensor2img of the fp32 restatement's output on the host, up to one grey level on a rounding boundary."""
    dev = _dev()
    import yaml
    from super_resolution_amd import data as D, metrics as M, test as T
    cfg, sd, _, _ = R.load_case("a")
    torch.save({"params": sd}, tmp_path / "net.pth")
    sizes = [(40, 45), (36, 50)]
    for i, (h, w) in enumerate(sizes):
        D.write_image(M.tensor2img(synth.synth_input(30 + i, (1, 3, h, w))), str(tmp_path / "lq" / f"im{i}.png"))
    opt = {"name": "ESC_RealM_toy_X2", "model_type": "ESRModel", "scale": 2, "num_gpu": 1,
           "datasets": {"test_1": {"name": "Toy", "type": "SingleImageDataset", "dataroot_lq": str(tmp_path / "lq"), "io_backend": {"type": "disk"}}},
           "network_g": dict(cfg, type="ESCRealM", attn_type="Naive", compute_dtype="fp32"),
           "path": {"pretrain_network_g": str(tmp_path / "net.pth"), "strict_load_g": True, "param_key_g": "params",
                    "visualization": str(tmp_path / "vis")},
           "val": {"save_img": True, "suffix": None}}
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    res = T.main(["-opt", str(tmp_path / "opt.yml")])
    assert len(res["Toy"]["images"]) == 2
    for i, (h, w) in enumerate(sizes):
        lq = D.read_image(str(tmp_path / "lq" / f"im{i}.png")).unsqueeze(0)
        xp = F.pad(lq, (0, (-w) % 32, 0, (-h) % 32), "reflect")
        want = M.tensor2img(R.forward(sd, cfg, xp)[:, :, :2 * h, :2 * w]).astype(np.int32)
        got = M.tensor2img(D.read_image(str(tmp_path / "vis" / "Toy" / f"im{i}_ESC_RealM_toy_X2.png")).unsqueeze(0)).astype(np.int32)
        assert got.shape == want.shape == (2 * h, 2 * w, 3)
        diff = np.abs(got - want)
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (int(diff.max()), float((diff > 0).mean()))
