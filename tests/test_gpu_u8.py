"""The 8-bit frame boundary on the GPU: uint8 frames in, uint8 frames out, through the kernels, the engine, the module, the
plans, the harness and the frame-sequence generator.  Expected values are computed here with torch on the CPU from the
reference's definitions (basicsr utils/img_util.py:9-35, :131; hat/models/hat_model.py:16-26, :110-112; img_util.py:66-91);
`metrics.tensor2img` is the yardstick for the output side."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from helpers import META, W_SEED, X_SEED, golden
from super_resolution_amd import metrics as M, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = [("HAT", n) for n in ("tiny_x2", "tiny_x4", "tiny_x3", "tiny_ocabesc_x2", "tiny_identity_ape_x2", "hats_1g_x4", "hat_1g_x2")] \
    + [("HATX", "hatx_tiny_plain_x2")]
HATS = dict(in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01, overlap_ratio=0.5,
            img_range=1.0, depths=[6] * 6, embed_dim=144, num_heads=[6] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _net(arch, name, dtype, dev, **kw):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    cfg = META["cfgs"][name] if isinstance(name, str) else name
    net = build_network(dict(type=arch, compute_dtype=dtype, **dict(cfg, **kw))).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    return net.to(dev)


def _img(t):
    """tensor2img per sample: (B,3,H,W) float -> (B,H,W,3) uint8"""
    return np.stack([M.tensor2img(t[i]) for i in range(t.shape[0])])


def _frames(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _float_path(net, frames, ws, s, dev):
    """read_image's float32(u8) / 255 as CHW -> pre_process (reflect-pad) -> net -> post_process (crop) -> tensor2img"""
    x = (frames.numpy().astype(np.float32) / np.float32(255.0))
    x = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
    h, w = x.shape[2:]
    ph, pw = (ws - h % ws) % ws, (ws - w % ws) % ws
    y = net(F.pad(x, (0, pw, 0, ph), "reflect").to(dev))
    return _img(y[:, :, :s * h, :s * w])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("pad", [(0, 0), (7, 0), (0, 7), (7, 7)])
def test_u8_to_planes_is_the_reflect_padded_quotient(pad, bgr):
    dev = _dev()
    from super_resolution_amd import ops
    B, h, w = 2, 37, 301                                       # not multiples of the 256-pixel workgroup row
    buf = _frames(11, (B, h, w + 5, 3))
    buf.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)   # every byte value is present
    src = buf.to(dev)[:, :, :w]                                 # pitch 3 (w + 5) > 3 w
    assert src.stride(1) == 3 * (w + 5)
    dst = torch.full((B, 3, h + pad[0], w + pad[1]), -1.0, device=dev)
    ops.u8_to_planes(src, dst, bgr=bgr)
    torch.cuda.synchronize()
    x = buf[:, :, :w].flip(-1) if bgr else buf[:, :, :w]
    ref = F.pad(x.permute(0, 3, 1, 2).to(torch.float32) / 255.0, (0, pad[1], 0, pad[0]), "reflect")
    assert len(torch.unique(buf[:, :, :w])) == 256
    assert torch.equal(dst.cpu(), ref)


# ---------------------------------------------------------------------------------------------- 2
def _special_planes(B, Hs, Ws):
    g = torch.Generator().manual_seed(5)
    t = torch.rand(B * 3 * Hs * Ws, generator=g) * 2.0 - 0.5
    k = torch.arange(256, dtype=torch.float32)
    half = (k[:255] + 0.5) / 255.0
    up, down = torch.nextafter(half, torch.tensor(2.0)), torch.nextafter(half, torch.tensor(-1.0))
    one = torch.tensor(1.0)
    sp = torch.cat([torch.tensor([-0.0, 0.0, 1.0, float(torch.nextafter(one, torch.tensor(2.0))), float("inf"), float("-inf")]),
                    k / 255.0, half, up, down, torch.nextafter(up, torch.tensor(2.0)), torch.nextafter(down, torch.tensor(-1.0))])
    assert sp.numel() <= Hs * Ws
    t[:sp.numel()] = sp
    return t.reshape(B, 3, Hs, Ws)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("crop", [(31, 61), (27, 57), (31, 50)])
def test_planes_to_u8_is_tensor2img(crop, bgr):
    dev = _dev()
    from super_resolution_amd import ops
    B, Hs, Ws = 2, 31, 61
    planes = _special_planes(B, Hs, Ws)
    ho, wo = crop
    buf = torch.full((B, ho, wo + 3, 3), 99, dtype=torch.uint8, device=dev)
    dst = buf[:, :, :wo]                                        # pitch 3 (wo + 3): odd for even wo, never a multiple of 4 bytes
    ops.planes_to_u8(planes.to(dev), dst, bgr=bgr)
    torch.cuda.synchronize()
    ref = _img(planes[:, :, :ho, :wo])
    assert np.array_equal(dst.cpu().numpy(), ref[..., ::-1] if bgr else ref)
    assert bool((buf[:, :, wo:] == 99).all()), "bytes between the rows are not the kernel's"
    packed = torch.empty(B, ho, wo, 3, dtype=torch.uint8, device=dev)   # the 4-byte-aligned store path
    ops.planes_to_u8(planes.to(dev), packed, bgr=bgr)
    assert np.array_equal(packed.cpu().numpy(), ref[..., ::-1] if bgr else ref)


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("W", [16, 48, 5120])
def test_conv3x3_to_u8_equals_planes_then_convert(W):
    dev = _dev()
    from super_resolution_amd import ops
    from super_resolution_amd.engine import RGB_MEAN
    B, H = 2, (37 if W < 5120 else 11)
    g = torch.Generator().manual_seed(W)
    x = (torch.randn(B, H, W, 64, generator=g)).to(torch.bfloat16).to(dev)
    wl = torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0)    # outputs spread over and beyond [0, 1] around the mean
    bl = torch.randn(3, generator=g) * 0.1
    wpk, b8 = ops.pack_cab_squeeze(wl, bl, dev)
    kw = dict(B=B, H=H, W=W, C_=64, ldx=64, out_scale=0.5, mean=RGB_MEAN, dtype=ops.HAT_BF16)
    planes = torch.empty(B, 3, H, W, device=dev)
    ops.conv3x3_to_planes(x, wpk, b8, planes, n_out=3, **kw)
    torch.cuda.synchronize()
    inside = float(((planes > 0) & (planes < 1)).float().mean())
    assert 0.3 < inside < 0.95, inside                           # neither all saturated nor all interior
    # crops that cut inside a 14-column strip, crops on a strip boundary, the full frame
    crops = {(H, W), (H - 3, W - 5), (H - 3, (W // 14) * 14 if W > 16 else 14), (1, 1), (H, W - 13)}
    for ho, wo in sorted(crops):
        for bgr in (False, True):
            ref = torch.empty(B, ho, wo, 3, dtype=torch.uint8, device=dev)
            ops.planes_to_u8(planes, ref, bgr=bgr)
            buf = torch.full((B, ho, wo + 1, 3), 77, dtype=torch.uint8, device=dev)
            out = buf[:, :, :wo]
            ops.conv3x3_to_u8(x, wpk, b8, out, h_out=ho, w_out=wo, bgr=bgr, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (W, ho, wo, bgr)
            assert bool((buf[:, :, wo:] == 77).all())


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c[1] for c in GOLDEN_CASES])
def test_forward_to_u8_is_tensor2img_of_forward(case, dtype):
    """Exact by construction (the same fp32 value, then the same three fp32 operations): no tolerance."""
    dev = _dev()
    arch, name = case
    g = golden(f"whole_{name}.npz")
    net = _net(arch, name, dtype, dev)
    x = synth.synth_input(X_SEED, tuple(g["x_shape"])).to(dev)
    y8 = net.forward_to_u8(x)
    ref = _img(net(x))
    assert y8.dtype == torch.uint8 and tuple(y8.shape) == ref.shape
    assert np.array_equal(y8.cpu().numpy(), ref)
    assert np.array_equal(net.forward_to_u8(x, bgr=True).cpu().numpy(), ref[..., ::-1])


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c[1] for c in GOLDEN_CASES])
def test_forward_to_u8_vs_reference_golden_f32(case):
    """Against the reference's own output y (whole_*.npz), fp32 engine, tol = 1e-4 (the project's fp32 parity bar).  A value is
    AT RISK when -tol < y < 1 + tol and 255 clip(y) lies within 255 tol + ulp(255) of a half-integer: there the 8-bit level may
    differ by one; everywhere else it must equal tensor2img(y).  The at-risk share must stay <= 5 % and >= 40 % of the values
    must lie strictly inside (0, 1), so that this is not a comparison of saturated pixels."""
    dev = _dev()
    arch, name = case
    g = golden(f"whole_{name}.npz")
    y = torch.from_numpy(np.asarray(g["y"], dtype=np.float32))
    net = _net(arch, name, "f32", dev)
    got = net.forward_to_u8(synth.synth_input(X_SEED, tuple(g["x_shape"])).to(dev)).cpu().numpy().astype(np.int64)
    want = _img(y).astype(np.int64)
    tol = 1e-4
    yd = y.permute(0, 2, 3, 1).numpy().astype(np.float64)
    v = 255.0 * np.clip(yd, 0.0, 1.0)
    risk = (yd > -tol) & (yd < 1 + tol) & (np.abs(v - np.floor(v) - 0.5) <= 255.0 * tol + 2.0 ** -16)
    inside = float(((yd > 0) & (yd < 1)).mean())
    print(f"{name}: at risk {risk.mean():.4f}, inside (0,1) {inside:.4f}, levels differing {(got != want).mean():.5f}")
    assert risk.mean() <= 0.05 and inside >= 0.40, (risk.mean(), inside)
    assert np.array_equal(got[~risk], want[~risk])
    assert np.abs(got - want)[risk].max(initial=0) <= 1


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [("HAT", "tiny_x2", (1, 37, 53)), ("HAT", "tiny_x3", (1, 16, 9)), ("HATX", "hatx_tiny_plain_x2", (2, 37, 53)),
                                  ("HAT", "hats_1g_x4", (1, 70, 41)), ("HAT", "hat_1g_x2", (2, 70, 41))],
                         ids=["tiny_x2_37x53", "tiny_x3_16x9", "hatx_B2_37x53", "hats_x4_70x41", "hat_x2_B2_70x41"])
def test_forward_u8_on_odd_sizes(case, dtype):
    dev = _dev()
    arch, name, (B, h, w) = case
    cfg = META["cfgs"][name]
    net = _net(arch, name, dtype, dev)
    frames = _frames(h * w, (B, h, w, 3))
    ref = _float_path(net, frames, cfg["window_size"], cfg["upscale"], dev)
    out = net.forward_u8(frames.to(dev))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, cfg["upscale"] * h, cfg["upscale"] * w, 3)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(net.forward_u8(frames.flip(-1).to(dev), bgr=True).cpu().numpy(), ref[..., ::-1])
    if B == 1:                                                   # (h,w,3) is accepted as one frame
        assert np.array_equal(net.forward_u8(frames[0].to(dev)).cpu().numpy(), ref)
    eng = net.engine()
    ws, s = cfg["window_size"], cfg["upscale"]
    n, key = eng.ws_allocations, (B, -(-h // ws) * ws, -(-w // ws) * ws)
    staged = eng._workspace(*key)["x_u8"]
    assert tuple(staged.shape) == (B, 3) + key[1:] and staged.dtype == torch.float32
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    out2 = net.forward_u8(frames.to(dev))
    torch.cuda.synchronize()
    assert eng.ws_allocations == n and eng._workspace(*key)["x_u8"] is staged, "the padded input lives in the per-shape workspace"
    assert torch.cuda.memory_allocated(dev) - before <= out2.numel() + 1024, "a call keeps nothing but its uint8 result"


def test_forward_u8_refusals():
    dev = _dev()
    net = _net("HAT", "tiny_x2", "f32", dev)
    with pytest.raises(RuntimeError, match="reflect"):
        net.forward_u8(torch.zeros(4, 20, 3, dtype=torch.uint8, device=dev))      # 4 rows cannot be padded to 8
    with pytest.raises(RuntimeError, match="uint8"):
        net.forward_u8(torch.zeros(1, 16, 16, 3, device=dev))
    net1 = _net("HAT", "tiny_x2", "f32", dev, in_chans=1)
    with pytest.raises(RuntimeError, match="in_chans"):
        net1.forward_u8(torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="in_chans"):
        net1.forward_to_u8(torch.zeros(1, 1, 16, 16, device=dev))


# ---------------------------------------------------------------------------------------------- 7
def test_720p_headline_takes_the_fused_epilogue_and_never_holds_the_float_image():
    dev = _dev()
    net = _net("HAT", HATS, "bf16", dev, upscale=4)
    eng = net.engine()
    image_bytes = 3 * 2880 * 5120 * 4
    for h, w in ((720, 1280), (718, 1275)):
        frames = _frames(h + w, (1, h, w, 3))
        ref = _float_path(net, frames, 16, 4, dev)
        d = frames.to(dev)
        fused, planes = eng.u8_fused_calls, eng.u8_planes_calls
        out = net.forward_u8(d)
        torch.cuda.synchronize()
        assert (eng.u8_fused_calls, eng.u8_planes_calls) == (fused + 1, planes), "conv_last converts in its epilogue"
        assert np.array_equal(out.cpu().numpy(), ref)
        del out
        out8 = torch.zeros(1, 4 * h, 4 * w, 3, dtype=torch.uint8, device=dev)   # the caller's result tensor, as a frame loop holds it
        x = torch.zeros(1, 3, 720, 1280, device=dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        y = net(x)
        torch.cuda.synchronize()
        peak_f = torch.cuda.max_memory_allocated(dev) - base
        del y
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        net.forward_u8(d, out=out8)
        torch.cuda.synchronize()
        peak_u = torch.cuda.max_memory_allocated(dev) - base
        assert np.array_equal(out8.cpu().numpy(), ref)
        print(f"{h}x{w}: peak above the resident set: forward {peak_f / 1e6:.1f} MB, forward_u8 {peak_u / 1e6:.1f} MB")
        assert peak_u <= peak_f - image_bytes, (peak_f, peak_u)   # the fp32 image is never allocated


# ---------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("case", [("HAT", "hats_1g_x4", "bf16", (1, 3, 32, 48), (27, 41)), ("HATX", "hatx_tiny_plain_x2", "f32", (2, 3, 16, 24), (13, 19))],
                         ids=["hats_bf16", "hatx_f32_B2"])
def test_plan_forward_u8(case, tmp_path):
    dev = _dev()
    from super_resolution_amd import plan
    arch, name, dtype, shape, small = case
    B, _, H, W = shape
    s = META["cfgs"][name]["upscale"]
    net = _net(arch, name, dtype, dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, shape, path)
    p = plan.Plan(path)
    stream = torch.cuda.current_stream().cuda_stream
    for h, w in ((H, W), small):                                 # the smaller frame pads to the plan's shape, as forward_u8 pads it
        frames = _frames(h + w, (B, h, w, 3)).to(dev)
        for bgr in (False, True):
            ref = net.forward_u8(frames, bgr=bgr)
            out = torch.full((B, s * h, s * w, 3), 9, dtype=torch.uint8, device=dev)
            p.forward_u8(frames, out, bgr=bgr, stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (h, w, bgr)
    from super_resolution_amd import _lib
    f = _frames(3, (B, H // 2, W, 3)).to(dev)                     # H - h >= h: no row to reflect
    assert _lib.load().hat_plan_forward_u8(p._h, f.data_ptr(), 3 * W, H // 2, W, f.data_ptr(), 3 * W * s, 0, stream) == -1
    assert _lib.load().hat_plan_forward_u8(p._h, f.data_ptr(), 3 * W + 3, H + 1, W, f.data_ptr(), 3 * W * s, 0, stream) == -1
    g = _frames(4, (B, H, W, 3)).to(dev)                          # a destination row does not fit its pitch
    assert _lib.load().hat_plan_forward_u8(p._h, g.data_ptr(), 3 * W, H, W, g.data_ptr(), 3 * W * s - 1, 0, stream) == -1
    x = synth.synth_input(X_SEED + 1, shape).to(dev)              # the float entry point is what it was
    y = torch.full((B, 3, H * s, W * s), 5.0, device=dev)
    p.forward(x, y, stream)
    torch.cuda.synchronize()
    assert torch.equal(y, net(x))
    p.close()


def _write_ppm(path, a):
    with open(path, "wb") as f:
        f.write(b"P6\n# written by the test\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())


def test_c_program_upscales_a_ppm(tmp_path):
    dev = _dev()
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from super_resolution_amd import plan
    exe = tmp_path / "plan_upscale_u8"
    r = subprocess.run(["gcc", os.path.join(ROOT, "examples", "plan_upscale_u8.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    net = _net("HAT", "hats_1g_x4", "bf16", dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, (1, 3, 32, 48), path)
    frame = _frames(8, (1, 29, 45, 3))
    want = net.forward_u8(frame.to(dev))[0].cpu().numpy()
    _write_ppm(tmp_path / "in.ppm", frame[0].numpy())
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), path, str(tmp_path / "in.ppm"), str(tmp_path / "out.ppm")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (tmp_path / "out.ppm").read_bytes()
    head = b"P6\n%d %d\n255\n" % (want.shape[1], want.shape[0])
    assert raw.startswith(head)
    assert np.array_equal(np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(want.shape), want)


# ---------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("tile", [None, {"tile_size": 32, "tile_pad": 16}], ids=["whole", "tiled"])
def test_harness_u8_on_device_writes_the_same_pngs_and_metrics(tmp_path, tile, dtype):
    dev = _dev()
    from PIL import Image
    from super_resolution_amd import data as D
    from super_resolution_amd.models import HATModel
    netopt = dict(type="HAT", upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=4, squeeze_factor=4, conv_scale=0.01,
                  overlap_ratio=0.5, img_range=1.0, depths=[2], embed_dim=24, num_heads=[2], mlp_ratio=2, upsampler="pixelshuffle",
                  resi_connection="1conv", compute_dtype=dtype)
    for i, (h, w) in enumerate([(45, 38), (33, 67), (50, 31)]):
        D.write_image(_frames(60 + i, (h, w, 3)).numpy(), str(tmp_path / "lq" / f"im{i}.png"))
        D.write_image(_frames(70 + i, (2 * h, 2 * w, 3)).numpy(), str(tmp_path / "gt" / f"im{i}.png"))
    from oracle import hat_oracle as O
    cfg = O.make_cfg(**{k: v for k, v in netopt.items() if k not in ("type", "compute_dtype")})
    torch.save({"params": synth.synth_state_dict(O.blank_state_dict(cfg), 21)}, tmp_path / "net.pth")
    ds = D.FolderDataset({"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"), "dataroot_lq": str(tmp_path / "lq"),
                          "scale": 2, "phase": "test"})
    results = {}
    for u8 in (False, True):
        opt = {"name": "toy", "scale": 2, "network_g": dict(netopt), "path": {"visualization": str(tmp_path / f"vis{int(u8)}"), "pretrain_network_g": str(tmp_path / "net.pth")},
               "val": {"suffix": None, "metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 2, "test_y_channel": True},
                                                   "ssim": {"type": "calculate_ssim", "crop_border": 2, "test_y_channel": True}}}}
        if u8:
            opt["val"]["u8_on_device"] = True
        if tile:
            opt["tile"] = tile
        model = HATModel(opt, device=str(dev))
        results[u8] = model.nondist_validation(ds, save_img=True)
    assert results[True] == results[False]
    for i in range(3):
        a, b = (np.asarray(Image.open(str(tmp_path / f"vis{k}" / "Toy" / f"im{i}_toy.png"))) for k in (0, 1))
        assert a.shape == b.shape and a.shape[2] == 3 and np.array_equal(a, b)


def test_harness_u8_input_planes_are_the_float_path_planes():
    """What the tiled u8 route feeds tile_process is, bit for bit, what pre_process makes of read_image's tensor: all 256 byte
    values, odd sizes, so a division that is not exact (a reciprocal multiply) cannot hide behind the network's rounding."""
    dev = _dev()
    from super_resolution_amd.models import HATModel
    netopt = dict(type="HAT", upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=4, squeeze_factor=4, conv_scale=0.01,
                  overlap_ratio=0.5, img_range=1.0, depths=[1], embed_dim=24, num_heads=[2], mlp_ratio=2, upsampler="pixelshuffle",
                  resi_connection="1conv", compute_dtype="f32")
    model = HATModel({"name": "toy", "scale": 2, "network_g": netopt, "path": {}, "tile": {"tile_size": 32, "tile_pad": 16}}, device=str(dev))
    frame = _frames(9, (1, 45, 38, 3))
    frame.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    lq = torch.from_numpy(frame.numpy().astype(np.float32) / np.float32(255.0)).permute(0, 3, 1, 2).contiguous()   # read_image
    model.feed_data({"lq": lq})
    model.pre_process()
    want, pads = model.img.clone(), (model.mod_pad_h, model.mod_pad_w)
    model.pre_process_u8(frame.to(dev))
    torch.cuda.synchronize()
    assert (model.mod_pad_h, model.mod_pad_w) == pads == (3, 10)
    assert torch.equal(model.img, want)


# ---------------------------------------------------------------------------------------------- 10
def test_upscale_frames_matches_forward_u8_in_order():
    dev = _dev()
    from super_resolution_amd import frames as FR
    net = _net("HAT", dict(HATS, depths=[2], num_heads=[6]), "bf16", dev, upscale=2)
    seq = [_frames(100 + i, (45, 70, 3)).numpy() for i in range(7)]
    assert len({a.tobytes() for a in seq}) == 7
    want = [net.forward_u8(torch.from_numpy(a).to(dev))[0].cpu().numpy() for a in seq]
    got = list(FR.upscale_frames(net, iter(seq)))
    assert len(got) == 7
    for i in range(7):
        assert got[i].dtype == np.uint8 and np.array_equal(got[i], want[i]), f"frame {i}"
    one = list(FR.upscale_frames(net, seq[:1], bgr=True))
    assert len(one) == 1 and np.array_equal(one[0], net.forward_u8(torch.from_numpy(seq[0]).to(dev), bgr=True)[0].cpu().numpy())
    assert list(FR.upscale_frames(net, [])) == []
    side = torch.cuda.Stream(device=dev)                          # the caller switches stream between frames
    gen, got2 = FR.upscale_frames(net, iter(seq[:4])), []
    for i in range(4):
        if i % 2:
            with torch.cuda.stream(side):
                got2.append(next(gen))
        else:
            got2.append(next(gen))
    assert next(gen, None) is None
    for i in range(4):
        assert np.array_equal(got2[i], want[i]), f"frame {i} with a switched stream"
