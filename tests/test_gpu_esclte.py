"""ESC-LTE on the device.  Kernel level: ops.lte_query (hat_lte_query) on synthetic coef / freq rows against the head of
tests/esclte_ref.py in fp64, both addressing modes, both dtypes, no query left out.  Whole model: forward, gen_feat + query_rgb over
the halves of the coordinates, and upscale against the reference's goldens (tests/golden/esclte_*.npz).

Bars, in image units (y * 0.5 + 0.5), README "Parity": fp32 max-abs <= 1e-4; bf16 >= 40 dB and max-abs <= 0.08.  At kernel level the
fp32 path is held to helpers.check's 2e-5 * max(scale, 1) against fp64 (what test_gpu_ops.py asks of hat_linear), and the two
addressing modes agree to it.  The bf16 instantiation is also judged on the MLP term alone (mlp_bar): got - base against the fp64
head with the MFMA weights rounded to bf16, minus base, where base is the fp64 bilinear base image — in the image bar the base of
an input with std 0.5 carries most of the signal.  Its bar is helpers.check's bf16 bar (relative L2 <= 1.2e-2); the measured
figures and the head with one 16-channel group dropped (tests/test_escreal_edges_ref_cpu.py) are in DESIGN 4.19."""
import functools

import pytest
import torch

import esclte_ref as R
from helpers import check, rnd

pytestmark = pytest.mark.gpu

DT = ["f32", "bf16"]
F32_IMG, BF16_DB, BF16_MAX = 1e-4, 40.0, 0.08


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def img_bar(got, ref, dtype, what):
    """The whole-model bars on y * 0.5 + 0.5; every query takes part."""
    got, ref = got.detach().double().cpu() * 0.5 + 0.5, torch.as_tensor(ref).double().cpu() * 0.5 + 0.5
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err, db = float((got - ref).abs().max()), R.psnr(got, ref)
    print(f"{what} [{dtype}]: max-abs {err:.3e}, {db:.1f} dB")
    if dtype == "f32":
        assert err <= F32_IMG, f"{what}: max-abs {err:.3e}"
    else:
        assert db >= BF16_DB and err <= BF16_MAX, f"{what}: {db:.1f} dB, max-abs {err:.3e}"


@functools.lru_cache(maxsize=None)
def head_case(H, W):
    """Synthetic rows of an H x W map: coef, freq ~ N(0, 1) (the goldens' conv outputs have that scale), a normalised input."""
    coef, freq = rnd(f"lte.coef{H}x{W}", (1, R.HIDDEN, H, W)), rnd(f"lte.freq{H}x{W}", (1, R.HIDDEN, H, W))
    inp = rnd(f"lte.inp{H}x{W}", (1, 3, H, W), std=0.5)
    return coef, freq, inp


@functools.lru_cache(maxsize=None)
def head_ref(H, W, key):
    """The fp64 head on the queries `key` names -> (coord, cell, y (Q,3) fp64); computed once, shared by both dtypes."""
    coef, freq, inp = head_case(H, W)
    if key[0] == "grid":
        coord, cell = R.grid_queries(key[1], (H, W), 4)
    else:
        coord, cell = R.scatter_queries(f"lte.q{H}x{W}.{key[1]}", key[1], HW=(H, W))
    y = R.head(R.d64(R.head_state_dict()), coef.double(), freq.double(), inp.double(), coord[None].double(), cell[None].double())[0]
    return coord, cell, y


@functools.lru_cache(maxsize=None)
def mlp_ref(H, W, key):
    """-> (the MLP term of the fp64 head whose three 256 x 256 layers are rounded to bf16, the fp64 base image), each (Q,3)."""
    coef, freq, inp = head_case(H, W)
    coord, cell, _ = head_ref(H, W, key)
    sd = R.d64(R.mfma_weights_as_bf16(R.head_state_dict()))
    base = R.bilinear_base(inp.double(), coord[None].double())[0]
    y = R.head(sd, coef.double(), freq.double(), inp.double(), coord[None].double(), cell[None].double())[0]
    return y - base, base


def mlp_bar(got, H, W, key, what):
    """The bf16 kernel's MLP term on its own: (got - base) against (ref - base) at helpers.check's bf16 bar."""
    ref, base = mlp_ref(H, W, key)
    term = got.detach().double().cpu() - base
    rel = float((term - ref).norm() / ref.norm())
    print(f"{what} [bf16] MLP term: rel {rel:.3e}, max-abs {float((term - ref).abs().max()):.3e} (scale {float(ref.abs().max()):.3g}, "
          f"base scale {float(base.abs().max()):.3g})")
    check(term, ref, "bf16", what + ", MLP term")


def device_head(dtype, H, W):
    from super_resolution_amd import ops
    dev = _dev()
    dt = ops.DTYPE_CODE[dtype]
    coef, freq, inp = head_case(H, W)
    rows = torch.cat([coef[0].reshape(R.HIDDEN, -1).t(), freq[0].reshape(R.HIDDEN, -1).t()], 1).contiguous().to(dev)   # (H*W, 512)
    pl = ops.pack_lte(R.head_state_dict(), dt, dev)
    kw = dict(H=H, W=W, ldc=2 * R.HIDDEN, ldf=2 * R.HIDDEN, dtype=dt)
    return ops, pl, rows, rows.view(-1)[R.HIDDEN:], inp[0].contiguous().to(dev), kw


def kernel_bar(got, ref, dtype, what):
    if dtype == "f32":
        check(got, ref, "f32", what)
    img_bar(got, ref, dtype, what)


MAPS = [(5, 7), (1, 3)]
GRIDS = {(5, 7): [(11, 13), (5, 7), (26, 35)], (1, 3): [(4, 7)]}   # (5,7): x2.2 / x1.86, x1, x5.2 / x5 (the cell clip)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_query_explicit(hw, dtype):
    """Explicit mode: Q = 1, one tile + 1 (33), and 143 scattered coordinates with -1 and 1 on both axes."""
    H, W = hw
    ops, pl, coef, freq, inp, kw = device_head(dtype, H, W)
    assert ops.LTE_TILE == 32
    for Q in (1, ops.LTE_TILE + 1, R.N_SCATTER):
        coord, cell, y = head_ref(H, W, ("scatter", Q))
        out = torch.full((Q, 3), float("nan"), device=coef.device)
        ops.lte_query(pl, coef, freq, inp, out, coord=coord.to(coef.device), cell=cell.to(coef.device), **kw)
        torch.cuda.synchronize()
        kernel_bar(out, y, dtype, f"lte_query explicit Q={Q} on {H}x{W}")
        if dtype == "bf16":
            mlp_bar(out, H, W, ("scatter", Q), f"lte_query explicit Q={Q} on {H}x{W}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_query_grid_equals_explicit(hw, dtype):
    """Grid mode (coordinates and cells made in the kernel, planes out, the affine applied) against the fp64 head, and against
    explicit mode on make_coord's coordinates: the two modes agree to the fp32 bar."""
    H, W = hw
    ops, pl, coef, freq, inp, kw = device_head(dtype, H, W)
    for h, w in GRIDS[hw]:
        coord, cell, y = head_ref(H, W, ("grid", (h, w)))
        planes = torch.full((3, h, w), float("nan"), device=coef.device)
        ops.lte_query(pl, coef, freq, inp, planes, grid=(h, w), cell_yx=(float(cell[0, 0]), float(cell[0, 1])), out_affine=(0.5, 0.5), **kw)
        rows = torch.full((h * w, 3), float("nan"), device=coef.device)
        ops.lte_query(pl, coef, freq, inp, rows, coord=coord.to(coef.device), cell=cell.to(coef.device), **kw)
        torch.cuda.synchronize()
        got = (planes.permute(1, 2, 0).reshape(-1, 3) - 0.5) / 0.5
        kernel_bar(got, y, dtype, f"lte_query grid {h}x{w} on {H}x{W}")
        if dtype == "bf16":
            mlp_bar(got, H, W, ("grid", (h, w)), f"lte_query grid {h}x{w} on {H}x{W}")
        check(got, rows, "f32", f"grid mode vs explicit mode {h}x{w} on {H}x{W} [{dtype}]")


# ------------------------------------------------------------------------------------------------
# whole model
# ------------------------------------------------------------------------------------------------
def _net(name, dtype):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    dev = _dev()
    cfg, sd, g, meta = R.load_case(name)
    net = build_network(dict(type="ESCLTE", **cfg, compute_dtype=dtype)).eval()
    net.load_state_dict(sd, strict=True)
    return net.to(dev), {k: torch.from_numpy(v).to(dev) for k, v in g.items()}, meta


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", list(R.CASES))
def test_model_against_the_reference(name, dtype):
    """forward; gen_feat + two query_rgb calls over the halves (equal to the one call); upscale on the grid cases."""
    net, g, meta = _net(name, "fp32" if dtype == "f32" else dtype)
    coord, cell = g["coord"][None], g["cell"][None]
    y = net(g["x"], coord, cell)
    assert tuple(y.shape) == (1, coord.shape[1], 3) and y.dtype == torch.float32
    img_bar(y[0], g["y"], dtype, f"ESCLTE {name} forward")
    feat = net.gen_feat(g["x"])
    assert tuple(feat.shape) == (1, 64, *g["x"].shape[-2:]) and feat.dtype == torch.float32 and torch.isfinite(feat).all()
    half = coord.shape[1] // 2 + 1
    y2 = torch.cat([net.query_rgb(coord[:, :half], cell[:, :half]), net.query_rgb(coord[:, half:], cell[:, half:])], 1)
    assert torch.equal(y2, y), "two query_rgb calls over the halves differ from the one call"
    if "grid" in meta["what"]:
        h, w = meta["what"]["grid"]
        up = net.upscale(g["x"] * 0.5 + 0.5, size=(h, w), scale_max=meta["what"]["scale_max"])
        assert tuple(up.shape) == (1, 3, h, w) and up.dtype == torch.float32
        img_bar((up[0].permute(1, 2, 0).reshape(-1, 3) - 0.5) / 0.5, g["y"], dtype, f"ESCLTE {name} upscale")
        if name == "a":
            assert tuple(net.upscale(g["x"] * 0.5 + 0.5, scale=1.5).shape) == (1, 3, 30, 36)


@pytest.mark.parametrize("dtype", DT)
def test_second_gen_feat_at_another_shape(dtype):
    """A query after a second gen_feat reads the new features: a 24x20 frame (case a's, transposed) after the 20x24 one."""
    net, g, _ = _net("a", "fp32" if dtype == "f32" else dtype)
    cfg, sd, _, _ = R.load_case("a")
    net.gen_feat(g["x"])
    x2 = g["x"].transpose(2, 3).contiguous()
    coord, cell = R.scatter_queries("esclte_second", 40, HW=(24, 20))
    want = R.forward(sd, cfg, x2.cpu(), coord[None], cell[None])[0]
    net.gen_feat(x2)
    got = net.query_rgb(coord[None].to(x2.device), cell[None].to(x2.device))[0]
    img_bar(got, want, dtype, "ESCLTE query after a second gen_feat")
    assert net.engine(x2.device).ws_allocations == 2


def test_command_line_writes_what_upscale_gives(tmp_path):
    """python -m super_resolution_amd.arb, in process: a checkpoint dict of the reference's form, one LR image, --size 31 40."""
    import numpy as np
    from PIL import Image
    from super_resolution_amd import arb, data
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    dev = _dev()
    sd = R.lte_state_dict(R.template_from_surface(R.surfaces()["surfaces"]["ESC_LTE"]["surface"]))
    ckpt = {"model": dict(name="lte", sd=sd, args=dict(encoder_spec=dict(name="esc", args=dict(no_upsampling=True)), hidden_dim=256,
                                                       imnet_spec=dict(name="mlp", args=dict(out_dim=3, hidden_list=[256, 256, 256]))))}
    torch.save(ckpt, tmp_path / "ckpt.pth")
    (tmp_path / "in").mkdir()
    u8 = np.random.default_rng(7).integers(0, 256, (20, 24, 3), dtype=np.uint8)
    Image.fromarray(u8, "RGB").save(tmp_path / "in" / "a.png")
    assert arb.main(["--model", str(tmp_path / "ckpt.pth"), "--input-path", str(tmp_path / "in"), "--output-path", str(tmp_path / "out"),
                     "--size", "31", "40", "--is-lr", "--compute-dtype", "fp32"]) == 0
    got = np.asarray(Image.open(tmp_path / "out" / "a.png").convert("RGB"))
    net = ESCLTE.from_checkpoint(ckpt, compute_dtype="fp32").to(dev)
    y = net.upscale(data.read_image(str(tmp_path / "in" / "a.png"))[None].to(dev), size=(31, 40))[0]
    want = y.clamp(0, 1).mul(255).byte().permute(1, 2, 0).cpu().numpy()
    assert got.shape == (31, 40, 3) and np.array_equal(got, want)
