"""ESC-LTE without a GPU: the restatement (tests/esclte_ref.py) against the reference's goldens, the registry, the constructor and the
state_dict surface against the reference's (esclte_surface.json), from_checkpoint, the pack-time refusals, the argument errors of the
calls, the inherited refusals, the packing of the head, and the symbol, signature and argument contract of hat_lte_query."""
import ctypes as C
import inspect

import pytest
import torch

import esclte_ref as R
from helpers import max_abs

KW = dict(R.ENC, n_blocks=1, conv_blocks=1)


def _build(**kw):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    return build_network(dict(type="ESCLTE", **kw))


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference(name):
    """fp32, the reference's operation order, and fp64: both within 1e-5 of what the reference gave."""
    cfg, sd, g, meta = R.load_case(name)
    x, coord, cell = (torch.from_numpy(g[k]) for k in ("x", "coord", "cell"))
    want_coord, want_cell = R.case_queries(name)
    assert torch.equal(coord, want_coord) and torch.equal(cell, want_cell) and tuple(x.shape) == tuple(meta["frame"])
    y32 = R.forward(sd, cfg, x, coord[None], cell[None])[0]
    assert tuple(y32.shape) == g["y"].shape == (coord.shape[0], 3)
    assert max_abs(y32, g["y"]) <= 1e-5
    y64 = R.forward(R.d64(sd), cfg, x.double(), coord[None].double(), cell[None].double())[0]
    assert max_abs(y64, g["y"]) <= 1e-5


@pytest.mark.parametrize("hw", [(1, 1), (3, 1)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_head_restatement_on_one_pixel_and_one_column_maps(hw):
    """The maps tests/test_gpu_escreal_edges.py adds, at its queries: the fp64 head agrees with the fp32 head in the reference's
    operation order (no query sits on a nearest-pixel tie the two would resolve differently), and on the 1 x 1 map with the closed
    form: all four shifts read the one pixel, rel = coord, the four areas are equal, the base is the pixel itself."""
    from test_gpu_esclte import head_case, head_ref
    from test_gpu_escreal_edges import LTE_EXPLICIT_Q, LTE_SMALL_MAPS
    H, W = hw
    coef, freq, inp = head_case(H, W)
    sd = R.head_state_dict()
    for key in (("scatter", LTE_EXPLICIT_Q), ("grid", LTE_SMALL_MAPS[hw])):
        coord, cell, y64 = head_ref(H, W, key)
        for ax in (0, 1):
            assert key[0] == "grid" or ((coord[:, ax] == -1).any() and (coord[:, ax] == 1).any())
        y32 = R.head(sd, coef, freq, inp, coord[None], cell[None])[0]
        assert tuple(y64.shape) == (coord.shape[0], 3) and max_abs(y32, y64) <= 2e-5
        if hw == (1, 1):
            c, k, fq = coord.double(), cell.double(), freq.double()[0, :, 0, 0]
            f = fq[0::2] * c[:, :1] + fq[1::2] * c[:, 1:] + k @ sd["phase.weight"].double().t()
            basis = coef.double()[0, :, 0, 0] * torch.cat([torch.cos(torch.pi * f), torch.sin(torch.pi * f)], -1)
            assert max_abs(R.imnet(R.d64(sd), basis) + inp.double()[0, :, 0, 0], y64) <= 1e-12


def test_golden_cases_are_what_the_issue_names():
    g = {n: R.load_case(n)[2] for n in R.CASES}
    assert g["a"]["coord"].shape[0] == 30 * 41 and g["b"]["coord"].shape[0] == 20 * 24 and g["c"]["coord"].shape[0] == 100 * 120
    assert g["d"]["coord"].shape[0] == 143
    for ax in (0, 1):
        assert (g["d"]["coord"][:, ax] == -1).any() and (g["d"]["coord"][:, ax] == 1).any()
    assert float(g["c"]["cell"][0, 0]) == pytest.approx(1.25 * 2 / 100) and float(g["a"]["cell"][0, 1]) == pytest.approx(2 / 41)
    # x1: the queries are the feature pixels' centres
    assert torch.equal(torch.from_numpy(g["b"]["coord"]), R.make_coord((20, 24)))


def test_upscale_restatement_is_forward_on_the_grid():
    cfg, sd, g, _ = R.load_case("a")
    img = torch.from_numpy(g["x"]) * 0.5 + 0.5
    y = R.upscale(sd, cfg, img, (30, 41))
    want = (torch.from_numpy(g["y"]) * 0.5 + 0.5).view(30, 41, 3).permute(2, 0, 1)[None]
    assert max_abs(y, want) <= 1e-5


def test_registry_round_trip():
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    from super_resolution_amd.registry import ARCH_REGISTRY
    import super_resolution_amd.archs as archs
    assert ARCH_REGISTRY.get("ESCLTE") is ESCLTE is archs.ESCLTE
    net = _build(**KW)
    assert isinstance(net, ESCLTE) and net.cfg["n_blocks"] == 1 and net.compute_dtype == "bf16" and net.use_graph is False


def test_constructor_signature_and_defaults():
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    p = list(inspect.signature(ESCLTE.__init__).parameters.values())[1:]
    assert [a.name for a in p] == ["dim", "pdim", "kernel_size", "n_blocks", "conv_blocks", "window_size", "num_heads", "exp_ratio", "hidden_dim",
                                   "hidden_list", "compute_dtype", "use_graph"]
    assert {a.name: a.default for a in p} == dict(dim=64, pdim=16, kernel_size=13, n_blocks=5, conv_blocks=5, window_size=32, num_heads=4,
                                                   exp_ratio=1.25, hidden_dim=256, hidden_list=(256, 256, 256), compute_dtype="bf16", use_graph=False)


@pytest.mark.parametrize("name", list(R.CASES) + ["ESC_LTE"])
def test_surface_key_for_key(name):
    meta = R.surfaces()
    ent = meta["cases"][name] if name in R.CASES else meta["surfaces"][name]
    net = _build(**ent["cfg"])
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == ent["surface"]
    keys = [k for k, _ in got]
    assert not any("to_img" in k or ".lns." in k or "rpe_idxs" in k for k in keys)
    assert ["phase.weight", [128, 2]] in got and "phase.bias" not in keys
    assert {f"imnet.layers.{i}.{p}" for i in (0, 2, 4, 6) for p in ("weight", "bias")} <= set(keys)
    if name == "ESC_LTE":
        assert sum(p.numel() for p in net.parameters()) == ent["nparams"]


def test_load_state_dict_is_a_plain_load():
    cfg, sd, _, _ = R.load_case("a")
    net = _build(**cfg)
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net.state_dict()["imnet.layers.6.weight"], sd["imnet.layers.6.weight"])
    with pytest.raises(RuntimeError, match="Missing key"):
        net.load_state_dict({k: v for k, v in sd.items() if k != "phase.weight"}, strict=True)


def _ckpt(sd=None, **over):
    model = dict(name="lte", args=dict(encoder_spec=dict(name="esc", args=dict(no_upsampling=True)),
                                       imnet_spec=dict(name="mlp", args=dict(out_dim=3, hidden_list=[256, 256, 256])), hidden_dim=256))
    model.update(over)
    if sd is not None:
        model["sd"] = sd
    return {"model": model}


def test_from_checkpoint_and_its_refusals():
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    meta = R.surfaces()["surfaces"]["ESC_LTE"]
    sd = R.lte_state_dict(R.template_from_surface(meta["surface"]))
    net = ESCLTE.from_checkpoint(_ckpt(sd), compute_dtype="fp32")
    assert net.cfg["n_blocks"] == net.cfg["conv_blocks"] == 5 and net.compute_dtype == "fp32" and not net.training
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    with pytest.raises(ValueError, match="'lte'"):
        ESCLTE.from_checkpoint(_ckpt(name="liif"))
    bad = _ckpt()
    bad["model"]["args"]["encoder_spec"]["name"] = "swinir"
    with pytest.raises(ValueError, match="swinir"):
        ESCLTE.from_checkpoint(bad)
    bad = _ckpt()
    bad["model"]["args"]["imnet_spec"]["name"] = "siren"
    with pytest.raises(ValueError, match="imnet_spec"):
        ESCLTE.from_checkpoint(bad)
    bad = _ckpt()
    bad["model"]["args"]["imnet_spec"] = None
    with pytest.raises(ValueError, match="imnet_spec"):
        ESCLTE.from_checkpoint(bad)


def test_pack_time_refusals():
    pack = lambda **kw: _build(**dict(KW, **kw))._make_engine("cpu")
    eng = pack()
    assert eng.lte.taps.nout == 512 and eng.lte.taps.ksize == 3 and not hasattr(eng, "to_img")
    with pytest.raises(ValueError, match="hidden_dim=128"):
        pack(hidden_dim=128, hidden_list=(128, 128, 128))
    with pytest.raises(ValueError, match=r"hidden_list=\(256, 256\)"):
        pack(hidden_list=(256, 256))
    with pytest.raises(ValueError, match=r"hidden_list=\(256, 128, 256\)"):
        pack(hidden_list=(256, 128, 256))
    with pytest.raises(ValueError, match="dim=48"):
        pack(dim=48)
    with pytest.raises(ValueError, match="window_size=16"):
        pack(window_size=16)
    with pytest.raises(ValueError, match="compute_dtype"):
        _build(**dict(KW, compute_dtype="fp16"))._make_engine("cpu")
    with pytest.raises(RuntimeError, match="one frame at a time"):
        eng._check_batch(2)
    with pytest.raises(RuntimeError, match="before gen_feat"):
        eng.query(torch.zeros(1, 2), torch.zeros(1, 2))


def test_head_packing_is_a_relayout():
    """hat_lte_query's operands (include/hat_mi355x.h): fragments [16][8][64][8] through packing.frags, the taps coef | freq."""
    from super_resolution_amd import ops, packing
    sd = R.head_state_dict()
    p = ops.pack_lte(sd, ops.HAT_F32, "cpu")
    for li, i in enumerate((0, 2, 4)):
        w = sd[f"imnet.layers.{i}.weight"]
        assert tuple(p.w[li].shape) == (16, 8, 64, 8) and torch.equal(p.w[li], packing.frags(w).contiguous())
        for t, ks, lane, j in [(0, 0, 0, 0), (15, 7, 63, 7), (3, 2, 17, 5), (9, 5, 40, 1), (1, 7, 15, 0), (14, 0, 48, 3)]:
            assert p.w[li][t, ks, lane, j] == w[16 * t + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
        assert torch.equal(p.b[li], sd[f"imnet.layers.{i}.bias"])
    assert torch.equal(p.w4, sd["imnet.layers.6.weight"]) and torch.equal(p.phase, sd["phase.weight"])
    assert p.taps.w.shape[0] == 512 and p.taps.w[256, 64 + 5] == sd["freq.weight"][0, 5, 0, 1] and p.taps.bias[255] == sd["coef.bias"][255]
    pb = ops.pack_lte(sd, ops.HAT_BF16, "cpu")
    assert pb.w[0].dtype == torch.bfloat16 and pb.w4.dtype == torch.float32 and pb.phase.dtype == torch.float32


def test_argument_errors_of_the_calls():
    net = _build(**KW).eval()
    img = torch.zeros(1, 3, 20, 24)
    with pytest.raises(ValueError, match="exactly one"):
        net.upscale(img)
    with pytest.raises(ValueError, match="exactly one"):
        net.upscale(img, size=(30, 40), scale=1.5)
    with pytest.raises(ValueError, match="empty"):
        net.upscale(img, scale=0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.upscale(img, scale=1.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.gen_feat(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(img, torch.zeros(1, 4, 2), torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match="before gen_feat"):
        net.query_rgb(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match="eval"):
        net.train().gen_feat(img)


def test_inherited_refusals():
    net = _build(**KW)
    for fn in ("forward_ensemble", "forward_to_u8", "forward_u8", "forward_gt_u8", "forward_yuv420", "forward_yuv"):
        with pytest.raises(NotImplementedError):
            getattr(net, fn)(None)
    with pytest.raises(NotImplementedError):
        net.forward_bands(None, 2)
    with pytest.raises(NotImplementedError):
        net.forward_band_parallel(None)


def test_hat_lte_query_symbol_and_signature():
    from super_resolution_amd import _lib
    import test_cabi_cpu
    assert "hat_lte_query" in test_cabi_cpu.header_functions()
    res, args = _lib.SIGNATURES["hat_lte_query"]
    assert res is C.c_int and len(args) == 28
    assert args == ([C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 11
                    + [C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p])
    lib = _lib.load()
    assert lib.hat_lte_query.argtypes == args and lib.hat_abi_version() == 2


def test_hat_lte_query_refuses_bad_arguments_without_a_device():
    """Every refusal below is decided from the arguments alone: no GPU is needed, and none is touched."""
    from super_resolution_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096)
    a = (buf.data_ptr() + 15) // 16 * 16
    base = dict(coef=a, freq=a + 1024, ldc=512, ldf=512, inp=a, H=2, W=2, phase=a, w1=a, b1=a, w2=a, b2=a, w3=a, b3=a, w4=a, b4=a, coord=a, cell=a,
                Q=5, gh=0, gw=0, cell_y=0.0, cell_x=0.0, out_a=1.0, out_b=0.0, out=a + 64, dtype=0)
    call = lambda **kw: lib.hat_lte_query(*dict(base, **kw).values(), None)
    for kw in [dict(coef=None), dict(freq=None), dict(inp=None), dict(phase=None), dict(w2=None), dict(b3=None), dict(w4=None), dict(b4=None),
               dict(out=None), dict(out=a), dict(coord=None), dict(cell=None), dict(Q=0), dict(H=0), dict(W=0), dict(H=65536, W=65536),
               dict(ldc=128), dict(ldf=258), dict(coef=a + 4), dict(w1=a + 8), dict(b2=a + 4), dict(phase=a + 8), dict(dtype=2),
               dict(coord=None, cell=None, gh=0, gw=8), dict(coord=None, cell=None, gh=8, gw=0), dict(coord=None, cell=None, gh=65536, gw=65536)]:
        assert call(**kw) == -1, kw


def test_command_line_sizes_and_the_host_shrink():
    """python -m super_resolution_amd.arb: inference.py:55-62's sizes, the refusals, and resize_fn's shrink through an 8-bit PIL image."""
    import numpy as np
    from PIL import Image
    from super_resolution_amd import arb
    assert arb.plan_sizes(20, 24, scale=1.5, size=None, is_lr=True) == (None, (30, 36))
    assert arb.plan_sizes(20, 24, scale=None, size=(31, 40), is_lr=True) == (None, (31, 40))
    assert arb.plan_sizes(21, 24, scale=2.0, size=None, is_lr=False) == ((10, 12), (21, 24))
    for kw in (dict(scale=None, size=None, is_lr=True), dict(scale=2.0, size=(4, 4), is_lr=True), dict(scale=1.5, size=None, is_lr=False),
               dict(scale=None, size=(30, 36), is_lr=False), dict(scale=32.0, size=None, is_lr=False)):
        with pytest.raises(ValueError):
            arb.plan_sizes(20, 24, **kw)
    with pytest.raises(SystemExit):
        arb.main(["--model", "m.pth", "--input-path", "in", "--output-path", "out", "--scale", "1.5"])   # fractional without --is-lr
    u8 = np.random.default_rng(5).integers(0, 256, (21, 24, 3), dtype=np.uint8)
    img = torch.from_numpy(u8.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)
    small = arb.shrink_like_the_reference(img, (10, 12))
    back = img.mul(255).byte().permute(1, 2, 0).numpy()    # ToPILImage truncates: a byte may come back one lower
    assert int(np.abs(back.astype(int) - u8.astype(int)).max()) <= 1
    want = np.asarray(Image.fromarray(back, "RGB").resize((12, 10), Image.BICUBIC), dtype=np.float32) / np.float32(255.0)
    assert tuple(small.shape) == (3, 10, 12) and np.array_equal(small.permute(1, 2, 0).numpy(), want)
