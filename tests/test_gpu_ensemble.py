"""The geometric self-ensemble on the GPU: hat_dihedral_f32 bit for bit against torch.flip / transpose on the CPU; the whole
model against goldens made with the reference's network (tests/golden/gen_golden_ensemble.py) under the project's bars;
forward_ensemble, the byte paths and the harness bit for bit against compositions of this build's own calls."""
import numpy as np
import pytest
import torch
import yaml

import ensemble_ref as E
from helpers import META, W_SEED, X_SEED, golden, max_abs
from oracle import hat_oracle as O
from super_resolution_amd import data as D, metrics as M, synth, yuv

pytestmark = pytest.mark.gpu

TILE = 64    # the kernel's tile side (csrc/hat_dihedral.hip)
SHAPES = [(3, 5, 37), (3, 33, 65), (1, 1, 7), (6, 64, 64), (3, 16, 24), (2, TILE + 1, TILE + 1), (1, 2 * TILE + 1, TILE + 6)]
CASES = {"tiny_x2": (1, 3, 16, 24), "tiny_x4": (1, 3, 24, 16), "hats_1g_x4": (1, 3, 16, 32)}


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


def _planes(shape, key="src"):
    return synth.normal(17, f"{key}{shape}", shape)


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_dihedral_is_flip_and_transpose_bit_for_bit(shape):
    dev = _dev()
    from super_resolution_amd import ops
    src = _planes(shape)
    d = src.to(dev)
    for op in range(8):
        out_shape = (shape[0], shape[2], shape[1]) if op & 4 else shape
        for inverse, ref in ((False, E.member(src, op)), (True, E.undo(src, op))):
            dst = torch.full(out_shape, float("nan"), device=dev)        # accumulate=0 overwrites: no stale read, every element written
            ops.dihedral(d, dst, op=op, inverse=inverse)
            torch.cuda.synchronize()
            assert torch.equal(dst.cpu(), ref), (op, inverse)
        # inverse(forward(x)) == x: tells members 5 and 6 apart
        fwd, back = torch.empty(out_shape, device=dev), torch.full(shape, float("nan"), device=dev)
        ops.dihedral(d, fwd, op=op)
        ops.dihedral(fwd, back, op=op, inverse=True)
        torch.cuda.synchronize()
        assert torch.equal(back.cpu(), src), op
    assert torch.equal(d.cpu(), src), "the source is read only"
    # anchors that do not go through ensemble_ref: member 3 is the half turn, 5 the counter-clockwise and 6 the clockwise quarter turn
    for op, k in ((3, 2), (5, 1), (6, -1)):
        dst = torch.empty((shape[0], shape[2], shape[1]) if op & 4 else shape, device=dev)
        ops.dihedral(d, dst, op=op)
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), torch.rot90(src, k, dims=(-2, -1))), op


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.125, 1.0 / 3.0, 0.3])
def test_dihedral_accumulate_is_the_fp32_expression(alpha):
    """dst + alpha * T(src) with the product and the sum each rounded to fp32, as torch computes the expression on the CPU.  For
    the powers of two the product is exact and a fused multiply-add gives the same bits; 1 / 3 and 0.3 are there to tell the
    two apart (the header promises the unfused result for every alpha)."""
    dev = _dev()
    alpha = float(torch.tensor(alpha, dtype=torch.float32))      # the fp32 value the C ABI receives
    from super_resolution_amd import ops
    for shape in ((3, 33, 65), (2, TILE + 1, TILE + 1)):
        src = _planes(shape)
        for op in range(8):
            out_shape = (shape[0], shape[2], shape[1]) if op & 4 else shape
            base = _planes(out_shape, "dst")
            for inverse, moved in ((False, E.member(src, op)), (True, E.undo(src, op))):
                dst = base.to(dev)
                ops.dihedral(src.to(dev), dst, op=op, inverse=inverse, alpha=alpha, accumulate=True)
                torch.cuda.synchronize()
                assert torch.equal(dst.cpu(), base + alpha * moved), (shape, op, inverse)
                if alpha not in (1.0, 0.5, 0.125):   # the case tells: one rounding (a fused multiply-add) gives other bits somewhere
                    assert not torch.equal((base.double() + alpha * moved.double()).float(), base + alpha * moved)
                plain = torch.full(out_shape, float("nan"), device=dev)
                ops.dihedral(src.to(dev), plain, op=op, inverse=inverse, alpha=alpha)
                torch.cuda.synchronize()
                assert torch.equal(plain.cpu(), alpha * moved), (shape, op, inverse)


def test_dihedral_wrapper_refusals():
    dev = _dev()
    from super_resolution_amd import ops
    x = torch.zeros(3, 16, 24, device=dev)
    with pytest.raises(RuntimeError, match="destination"):
        ops.dihedral(x, torch.zeros(3, 16, 24, device=dev), op=4)          # a transposing member needs (3, 24, 16)
    with pytest.raises(RuntimeError, match="destination"):
        ops.dihedral(x, torch.zeros(3, 24, 16, device=dev), op=3)
    with pytest.raises(RuntimeError, match="0..7"):
        ops.dihedral(x, torch.zeros(3, 16, 24, device=dev), op=8)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.dihedral(x, x, op=1)                                           # in place
    with pytest.raises(RuntimeError):
        ops.dihedral(x.half(), torch.zeros(3, 16, 24, device=dev), op=0)


# ---------------------------------------------------------------------------------------------- whole model vs the reference
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_ensemble_vs_reference_golden(name, dtype):
    dev = _dev()
    g = golden(f"ensemble_{name}.npz")
    net = _net("HAT", name, dtype, dev)
    x = synth.synth_input(X_SEED, CASES[name]).to(dev)
    for n in (8, 4):
        y = net.forward_ensemble(x, n)
        torch.cuda.synchronize()
        ref = torch.from_numpy(g[f"y{n}"])
        assert y.shape == ref.shape and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
        err, psnr = max_abs(y.cpu(), ref), O.psnr_float(y.cpu(), ref)
        print(f"ENSEMBLE-GOLDEN {name}/{dtype} n={n}: max-abs {err:.3e} PSNR {psnr:.2f} dB")
        if dtype == "f32":
            assert err <= 1e-4, (name, n, err)
        else:
            assert psnr >= 40.0 and err <= 0.08, (name, n, psnr, err)


def test_hatx_ensemble_vs_oracle_loop():
    dev = _dev()
    cfg = O.make_hatx_cfg(**META["cfgs"]["hatx_tiny_plain_x2"])
    sd = synth.synth_state_dict(O.hatx_blank_state_dict(cfg), W_SEED)
    x = synth.synth_input(X_SEED, (1, 3, 16, 24))
    ref = E.ensemble(lambda t: O.hatx_forward(t, sd, cfg), x, 8)
    net = _net("HATX", "hatx_tiny_plain_x2", "f32", dev)
    y = net.forward_ensemble(x.to(dev), 8)
    torch.cuda.synchronize()
    err = max_abs(y.cpu(), ref)
    print(f"ENSEMBLE-HATX f32: max-abs vs oracle loop {err:.3e}")
    assert y.shape == ref.shape and err <= 1e-4, err


# ---------------------------------------------------------------------------------------------- wiring, bit for bit
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_ensemble_is_the_composition(dtype):
    dev = _dev()
    net = _net("HAT", "tiny_x2", dtype, dev)
    x = synth.synth_input(X_SEED, (2, 3, 16, 24)).to(dev)
    plain = net(x)
    got = {}
    for n in (8, 4, 2):
        got[n] = net.forward_ensemble(x, n)
        ref = E.ensemble(net, x, n)        # the same members through this build's forward, moved and added by torch ops on the device
        torch.cuda.synchronize()
        assert torch.equal(got[n], ref), n
    assert not torch.equal(got[8], got[4]) and not torch.equal(got[4], got[2]) and not torch.equal(got[2], plain)
    one = net.forward_ensemble(x, 1)
    again = net.forward_ensemble(x, 8)
    torch.cuda.synchronize()
    assert torch.equal(one, plain) and one.data_ptr() != plain.data_ptr()
    assert torch.equal(again, got[8]) and again.data_ptr() != got[8].data_ptr() and torch.equal(net(x), plain), "no state is left behind"
    assert net.forward_ensemble(x.half(), 8).dtype == torch.float16


def test_forward_ensemble_refusals():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "f32", dev)
    x = torch.zeros(1, 3, 16, 24, device=dev)
    for bad in (0, 3, 16, True, None, "8"):
        with pytest.raises(ValueError):
            net.forward_ensemble(x, bad)
        with pytest.raises(ValueError):
            net.forward_u8(torch.zeros(19, 27, 3, dtype=torch.uint8, device=dev), ensemble=bad)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        net.forward_ensemble(x.cpu(), 8)
    for n in (8, 1):
        with pytest.raises(RuntimeError, match="multiple of window_size"):
            net.forward_ensemble(torch.zeros(1, 3, 16, 20, device=dev), n)
        with pytest.raises(RuntimeError, match=r"expected \(B,3,H,W\)"):
            net.forward_ensemble(torch.zeros(1, 4, 16, 24, device=dev), n)
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net.forward_ensemble(x, 8)
    net.eval()
    ape = _net("HAT", "tiny_identity_ape_x2", "f32", dev)
    size = META["cfgs"]["tiny_identity_ape_x2"]["img_size"]
    with pytest.raises(RuntimeError, match="absolute_pos_embed"):
        ape.forward_ensemble(torch.zeros(1, 3, size, size + 8, device=dev), 8)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_u8_ensemble_is_the_composition(dtype):
    """u8_to_planes with the reflect-pad -> forward_ensemble -> crop -> planes_to_u8, on a frame that needs padding; ensemble=1
    is today's call (on the bf16 path that is conv_last's fused epilogue, which the counters show)."""
    dev = _dev()
    from super_resolution_amd import ops
    net = _net("HAT", "tiny_x2", dtype, dev)
    h, w, ws, s = 19, 27, 8, 2
    frame = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, h, w, 3), dtype=np.uint8)).to(dev)
    x = torch.empty(1, 3, 24, 32, device=dev)
    ops.u8_to_planes(frame, x)
    y = net.forward_ensemble(x, 8)
    ref = torch.empty(1, s * h, s * w, 3, dtype=torch.uint8, device=dev)
    ops.planes_to_u8(y, ref)
    eng = net.engine()
    before = (eng.u8_fused_calls, eng.u8_planes_calls)
    got = net.forward_u8(frame, ensemble=8)
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and (eng.u8_fused_calls, eng.u8_planes_calls) == (before[0], before[1] + 1)
    out = torch.zeros_like(ref)
    assert net.forward_u8(frame[0], ensemble=8, out=out) is out and torch.equal(out, ref)
    bgr = net.forward_u8(frame.flip(-1), ensemble=8, bgr=True)
    assert torch.equal(bgr.flip(-1), ref)
    assert torch.equal(net.forward_to_u8(x, ensemble=8), net.forward_to_u8(x, ensemble=8)) and \
        torch.equal(net.forward_to_u8(x, ensemble=8)[:, :s * h, :s * w], ref)
    # ensemble=1: the call as it was
    today = net.forward_u8(frame)
    before = (eng.u8_fused_calls, eng.u8_planes_calls)
    one = net.forward_u8(frame, ensemble=1)
    torch.cuda.synchronize()
    fused = bool(eng.u8_fused)    # 2 * 32 output columns, a multiple of 16: where the row-sweep conv_last exists it converts in its epilogue
    assert fused == (dtype == "bf16")
    assert torch.equal(one, today) and (eng.u8_fused_calls, eng.u8_planes_calls) == (before[0] + int(fused), before[1] + int(not fused))
    assert not torch.equal(one, ref), "one forward and the ensemble of eight differ"


def test_forward_yuv420_ensemble_is_the_composition():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "f32", dev)
    h, w, ws, s = 18, 26, 8, 2
    frames = np.random.default_rng(6).integers(0, 256, (1,) + yuv.frame_shape(h, w), dtype=np.uint8)
    x = yuv.yuv420_to_planes(frames, fmt="nv12", pad=((ws - h % ws) % ws, (ws - w % ws) % ws))
    y = net.forward_ensemble(torch.from_numpy(x).to(dev), 4)
    ref = yuv.planes_to_yuv420(y.cpu().numpy(), fmt="nv12", crop=(s * h, s * w))
    d = torch.from_numpy(frames).to(dev)
    got = net.forward_yuv420(d, fmt="nv12", ensemble=4)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    today, one = net.forward_yuv420(d, fmt="nv12"), net.forward_yuv420(d, fmt="nv12", ensemble=1)
    assert torch.equal(today, one) and not torch.equal(one, got)


# ---------------------------------------------------------------------------------------------- the harness
NET = dict(type="HAT", upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=4, squeeze_factor=4, conv_scale=0.01,
           overlap_ratio=0.5, img_range=1.0, depths=[2], embed_dim=24, num_heads=[2], mlp_ratio=2, upsampler="pixelshuffle",
           resi_connection="1conv", compute_dtype="f32")
METRICS = {"psnr": {"type": "calculate_psnr", "crop_border": 2, "test_y_channel": True},
           "ssim": {"type": "calculate_ssim", "crop_border": 2, "test_y_channel": True}}
PSNR_Y_BAR, SSIM_BAR = 1e-8, 1e-10      # test_gpu_metrics.py's bars for device scores against host scores of the same bytes


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path)).convert("RGB"))


@pytest.mark.parametrize("tile", [None, {"tile_size": 32, "tile_pad": 16}], ids=["whole", "tiled"])
def test_harness_self_ensemble(tmp_path, tile):
    dev = _dev()
    import torch.nn.functional as F
    from super_resolution_amd import tile_parallel as tp
    from super_resolution_amd.models import HATModel
    from super_resolution_amd import test as T
    sizes = [(40, 36), (35, 52)]
    rng = np.random.default_rng(8)
    for i, (h, w) in enumerate(sizes):
        D.write_image(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), str(tmp_path / "lq" / f"im{i}.png"))
        D.write_image(rng.integers(0, 256, (2 * h, 2 * w, 3), dtype=np.uint8), str(tmp_path / "gt" / f"im{i}.png"))
    cfg = O.make_cfg(**{k: v for k, v in NET.items() if k not in ("type", "compute_dtype")})
    torch.save({"params": synth.synth_state_dict(O.blank_state_dict(cfg), 21)}, tmp_path / "net.pth")
    dataset = lambda: D.FolderDataset({"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"),
                                       "dataroot_lq": str(tmp_path / "lq"), "scale": 2, "phase": "test"})

    def options(vis, **val):
        opt = {"name": "toy", "scale": 2, "network_g": dict(NET), "path": {"visualization": str(tmp_path / vis), "pretrain_network_g": str(tmp_path / "net.pth")},
               "val": dict({"suffix": None, "metrics": METRICS}, **val)}
        if tile:
            opt["tile"] = tile
        return opt

    # the float branch, from a YAML file that says `self_ensemble: true`
    yml = tmp_path / "opt.yml"
    yml.write_text(yaml.safe_dump(options("vis_float", self_ensemble=True)))
    assert "self_ensemble: true" in yml.read_text()
    model = HATModel(T.parse_options(str(yml)), device=str(dev))
    assert model.ensemble == 8
    mean_f, rows_f = model.nondist_validation(dataset(), save_img=True)
    net = model.get_bare_model(model.net_g)
    for i, (h, w) in enumerate(sizes):
        lq = D.read_image(str(tmp_path / "lq" / f"im{i}.png")).unsqueeze(0).to(dev)
        img = F.pad(lq, (0, (16 - w % 16) % 16, 0, (16 - h % 16) % 16), "reflect")
        ens = lambda t: net.forward_ensemble(t, 8)
        y = tp.tile_forward(img, ens, 2, tp.reference_tiles(img.shape[2], img.shape[3], 32, 16)) if tile else ens(img)
        want = M.tensor2img(y[:, :, :2 * h, :2 * w].cpu())
        assert np.array_equal(_png(tmp_path / "vis_float" / "Toy" / f"im{i}_toy.png"), want), f"im{i}"
        assert not np.array_equal(want, M.tensor2img((tp.tile_forward(img, net, 2, tp.reference_tiles(img.shape[2], img.shape[3], 32, 16))
                                                      if tile else net(img))[:, :, :2 * h, :2 * w].cpu())), "the option changes the image"
    # the three byte branches write the same bytes; the device scores are the host scores of those PNGs
    for vis, val in (("vis_u8", dict(u8_on_device=True)), ("vis_dev", dict(metrics_on_device=True)),
                     ("vis_lq", dict(lq_on_device=True, metrics_on_device=True))):
        mean, rows = HATModel(options(vis, self_ensemble=8, **val), device=str(dev)).nondist_validation(dataset(), save_img=True)
        for i in range(len(sizes)):
            png = _png(tmp_path / vis / "Toy" / f"im{i}_toy.png")
            if vis != "vis_lq":      # (lq_on_device makes its own LQ image from the ground truth: another input)
                assert np.array_equal(png, _png(tmp_path / "vis_float" / "Toy" / f"im{i}_toy.png")), (vis, i)
            gt = _png(tmp_path / "gt" / f"im{i}.png")[:png.shape[0], :png.shape[1]]
            for name, bar in (("psnr", PSNR_Y_BAR), ("ssim", SSIM_BAR)):
                host = M.calculate_metric({"img": png, "img2": gt}, METRICS[name])
                print(f"ENSEMBLE-HARNESS {vis} im{i} {name}: harness {rows[i][name]!r} host {host!r}")
                assert abs(rows[i][name] - host) <= bar, (vis, i, name)
    # lq_on_device against its composition: imresize -> forward_ensemble (whole or per tile) -> planes_to_u8
    from super_resolution_amd import ops
    gt8 = torch.from_numpy(_png(tmp_path / "gt" / "im0.png").copy()).unsqueeze(0).to(dev)
    h, w = sizes[0]
    x = ops.imresize(gt8, 0.5, pad_to=(48, 48))
    y = tp.tile_forward(x, ens, 2, tp.reference_tiles(48, 48, 32, 16)) if tile else ens(x)
    want = torch.empty(1, 2 * h, 2 * w, 3, dtype=torch.uint8, device=dev)
    ops.planes_to_u8(y.contiguous(), want)
    assert np.array_equal(_png(tmp_path / "vis_lq" / "Toy" / "im0_toy.png"), want[0].cpu().numpy())
    # a value the harness does not know raises before the first image
    with pytest.raises(ValueError, match="self_ensemble"):
        HATModel(options("vis_bad", self_ensemble=3), device=str(dev)).nondist_validation(dataset(), save_img=True)
    assert not (tmp_path / "vis_bad").exists()


def test_upscale_frames_ensemble():
    dev = _dev()
    from super_resolution_amd import frames as FR
    net = _net("HAT", "tiny_x2", "bf16", dev)
    seq = [np.random.default_rng(20 + i).integers(0, 256, (19, 27, 3), dtype=np.uint8) for i in range(3)]
    got = list(FR.upscale_frames(net, iter(seq), ensemble=4))
    for a, g in zip(seq, got):
        assert np.array_equal(g, net.forward_u8(torch.from_numpy(a).to(dev), ensemble=4)[0].cpu().numpy())
    with pytest.raises(ValueError):
        next(FR.upscale_frames(net, iter(seq), ensemble=5))
