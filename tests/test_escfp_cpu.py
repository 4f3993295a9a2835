"""ESCFP without a GPU: the fp64 restatement (tests/escfp_ref.py) against the reference's goldens, the registry name, the constructor
and the state-dict surface against the reference's (tests/golden/escfp_surface.json), the `to_img` conversion, the pack-time errors,
and the algebra the device path rests on: the rank-1 fold of the decomposed large-kernel branch and the phase-table bicubic."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import esc_ref as E
import escfp_ref as R
from helpers import max_abs, rnd
from super_resolution_amd import _lib, packing
from super_resolution_amd.registry import ARCH_REGISTRY, build_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["a", "b", "c", "d"]


def _rows_at(t, px):
    """(B,C,H,W) -> (B, pixels, C) at the flat pixel indices px: the layout of the goldens' taps."""
    b, c = t.shape[:2]
    return t.reshape(b, c, -1)[:, :, torch.as_tensor(px)].permute(0, 2, 1)


@pytest.mark.parametrize("name", ALL)
def test_restatement_matches_the_reference_goldens(name):
    cfg, sd, g, meta = R.load_case(name)
    assert (cfg, tuple(meta["frame"])) == (R.CASES[name] if name != "d" else R.CASE_D)
    taps = {}
    x = torch.from_numpy(g["x"]).double()
    y = R.forward(R.d64(sd) if name != "d" else _converted(sd, cfg), cfg, x, taps=taps)
    assert list(y.shape) == list(g["y"].shape)
    if "tap_pixels" in g:
        assert np.array_equal(g["tap_pixels"], E.tap_pixels(*meta["frame"][2:]))
        for k in R.TAPS:
            assert g[k].shape == (meta["frame"][0], len(g["tap_pixels"]), 48)
            err = max_abs(_rows_at(taps[k], g["tap_pixels"]), g[k])
            assert err <= 1e-5, f"escfp_{name} {k}: max-abs {err:.3e}"
    err = max_abs(y, g["y"])
    print(f"escfp_{name}: restatement vs reference max-abs {err:.3e}")
    assert err <= 1e-5, f"escfp_{name}: max-abs {err:.3e}"
    # the folded (dense rank-1) form of the large-kernel branch gives the same network
    assert max_abs(R.forward(R.d64(sd) if name != "d" else _converted(sd, cfg), cfg, x, plk=R.plk_folded), y) <= 1e-9


def _converted(sd, cfg):
    sd = R.d64(sd)
    k, b = E.convert_to_img(sd["to_img.weight"].float(), sd["to_img.bias"].float(), cfg["upscaling_factor"])   # fp32, as load_state_dict
    return dict(sd, **{"to_img.weight": k.double(), "to_img.bias": b.double()})


def test_case_c_is_a_batch_of_two_different_images():
    _, _, g, meta = R.load_case("c")
    assert g["x"].shape[0] == 2 and max_abs(g["x"][0], g["x"][1]) > 0.5 and meta["batch_vs_single_max_abs"] <= 1e-5


def test_registry_name_and_constructor():
    from super_resolution_amd.archs import ESC, ESCFP
    from super_resolution_amd.archs.hat_arch import HAT
    cls = ARCH_REGISTRY.get("ESCFP")
    assert cls is ESCFP and issubclass(cls, HAT) and not issubclass(cls, ESC) and ESC.__mro__[1] is cls.__mro__[1]
    p = inspect.signature(cls.__init__).parameters
    ref = ["self", "dim", "pdim", "kernel_size", "n_blocks", "conv_blocks", "window_size", "num_heads", "upscaling_factor", "exp_ratio",
           "attn_type", "compute_dtype", "use_graph"]
    assert list(p) == ref
    assert (p["exp_ratio"].default, p["attn_type"].default, p["compute_dtype"].default, p["use_graph"].default) == (2, "Flex", "bf16", False)
    with pytest.raises(NotImplementedError):
        cls(**dict(R.CASES["a"][0], attn_type="Other"))
    net = cls(**R.CASES["b"][0])
    assert not hasattr(net, "convert") and not hasattr(net, "plk_filter") and net.upscale == net.upscaling_factor == 4
    assert ARCH_REGISTRY.get("ESC") is ESC


@pytest.mark.parametrize("name", ["a", "b", "c"] + list(R.SURFACE_CFGS))
def test_state_dict_surface_equals_the_reference(name):
    meta = R.surfaces()
    m = meta["cases"][name] if name in R.CASES else meta["surfaces"][name]
    net = build_network(dict(m["cfg"], type="ESCFP", attn_type="Naive"))
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == m["surface"]
    assert {"lk_channel", "lk_spatial", "blocks.0.pconvs.0.plk.proj.1.weight", "blocks.0.pconvs.0.plk.proj.3.bias", "blocks.0.lns.0.weight",
            "ln_last.weight", "ln_last.bias"} <= set(sd)
    assert tuple(sd["lk_channel"].shape) == (16, 16, 1, 1) and tuple(sd["lk_spatial"].shape) == (16, 1, 13, 13)
    assert tuple(sd["blocks.0.pconvs.0.plk.proj.1.weight"].shape) == (4, 16, 1, 1) and tuple(sd["blocks.0.proj.proj.weight"].shape) == (72, 48, 1, 1)
    if name in R.SURFACE_CFGS:
        assert sum(p.numel() for p in net.parameters()) == meta["nparams"][name]
        assert tuple(sd["blocks.4.convffns.4.proj.weight"].shape) == (60, 48, 1, 1)


def test_registry_round_trip_and_strict_load():
    cfg, sd, _, _ = R.load_case("a")
    net = build_network(dict(cfg, type="ESCFP", attn_type="Naive", compute_dtype="fp32"))
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if k != "ln_last.bias"}, strict=True)
    assert net.compute_dtype == "fp32" and net.cfg["use_ln"] is True


def test_load_state_dict_converts_to_img_of_another_scale():
    cfg, sd, _, _ = R.load_case("d")
    assert cfg["upscaling_factor"] == 4 and tuple(sd["to_img.weight"].shape) == (12, 48, 3, 3)
    net = build_network(dict(cfg, type="ESCFP"))
    net.load_state_dict(sd, strict=True)
    k, b = E.convert_to_img(sd["to_img.weight"], sd["to_img.bias"], 4)
    assert tuple(net.to_img.weight.shape) == (48, 48, 3, 3) and torch.equal(net.to_img.weight, k) and torch.equal(net.to_img.bias, b)
    assert tuple(sd["to_img.weight"].shape) == (12, 48, 3, 3), "the caller's dict was changed"
    from super_resolution_amd.archs import esc_arch, esc_fp_arch
    assert "load_state_dict" not in vars(esc_fp_arch.ESCFP) and "load_state_dict" not in vars(esc_arch.ESC)   # one copy of the conversion


# ---- the algebra ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(20, 23), (3, 5), (1, 1)])
def test_rank1_fold_equals_the_1x1_plus_depthwise_form_at_the_border_too(hw):
    lc, k = rnd("lc", (16, 16, 1, 1), std=0.25).double(), rnd("kk", (16, 1, 13, 13), std=1 / 13).double()
    x = rnd(f"fx{hw}", (1, 16) + hw).double()
    weff = packing.escfp_rank1_fold(lc, k)
    assert weff.dtype == torch.float64 and tuple(weff.shape) == (16, 16, 13, 13)
    want = F.conv2d(F.conv2d(x, lc), k, padding=6, groups=16)
    got = F.conv2d(x, weff, padding=6)
    assert max_abs(got, want) <= 1e-12 * max(1.0, float(want.abs().max()))
    if hw[0] > 1:   # a bias on the 1x1 breaks it at the border only: zero padding of the 1x1's output is not the 1x1 of a padded input
        bias = rnd("lcb", (16,)).double()
        two = F.conv2d(F.conv2d(x, lc, bias), k, padding=6, groups=16)
        one = F.conv2d(F.pad(x, (6, 6, 6, 6)), weff) + F.conv2d(F.pad(torch.ones_like(x), (6, 6, 6, 6)) * 0 + 1, k * bias.reshape(16, 1, 1, 1), groups=16)
        assert max_abs(one, two) > 1e-3


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (33, 40)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_phase_table_bicubic_matches_interpolate(s, hw):
    tab = packing.bicubic_phase_table(s)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (s, 4)
    assert max_abs(tab.double().sum(1), torch.ones(s)) <= 1e-7
    for p in range(s):   # phase p and s - 1 - p mirror each other (the centre phase of an odd factor is its own mirror, one tap over)
        assert 2 * p + 1 == s or torch.equal(tab[p], tab[s - 1 - p].flip(0))
    x = rnd(f"bx{hw}", (2, 3) + hw, std=0.3) + 0.5
    want = F.interpolate(x, scale_factor=s, mode="bicubic")
    got = R.bicubic_phase(x.double(), s, tab)
    assert got.shape == want.shape
    err = max_abs(got, want)
    assert err <= 1e-5, f"x{s} {hw}: {err:.3e}"
    if hw == (33, 40):
        mat = F.interpolate(x, scale_factor=s, mode="bilinear")
        assert max_abs(mat, want) > 1e-2   # (the comparison can tell two interpolations apart)


def test_phase_table_is_keys_with_a_minus_three_quarters():
    tab = packing.bicubic_phase_table(2).double()
    t, A = 0.75, -0.75
    w1 = ((A + 2) * t - (A + 3)) * t * t + 1
    assert abs(float(tab[0, 1]) - w1) <= 1e-7 and abs(float(tab[1, 2]) - w1) <= 1e-7
    assert torch.equal(packing.bicubic_phase_table(3)[1], torch.tensor([0.0, 1.0, 0.0, 0.0]))   # the odd factor's centre phase copies


# ---- packing --------------------------------------------------------------------------------------------------------------------
def test_convffn_packing_layout_at_48_channels():
    cfg, sd, _, _ = R.load_case("a")
    f = packing.pack_escfp_convffn(sd, "blocks.0.convffns.0", _lib.HAT_F32, "cpu")
    assert (f.hid, f.hid_p) == (60, 64) and f.w1.shape == (4, 2, 64, 8) and f.w2.shape == (3, 2, 64, 8) and f.dww.shape == (9, 64)
    W1, W2 = sd["blocks.0.convffns.0.proj.weight"].reshape(60, 48), sd["blocks.0.convffns.0.aggr.weight"].reshape(48, 60)
    t, ks, lane, j = 2, 1, 21, 5     # column 32 + 8 + 5 = 45 < 48
    assert f.w1[t, ks, lane, j] == W1[16 * t + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
    assert f.w2[t, ks, lane, j] == W2[16 * t + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
    assert float(f.w1[:, 1, 32:].abs().max()) == 0, "K columns 48..63 of W1 (lanes g >= 2 of the second k-step)"
    assert float(f.w1[3, :, 12:16].abs().max()) == 0 and float(f.w1[3, :, 28:32].abs().max()) == 0, "hidden units 60..63"
    assert float(f.b1[60:].abs().max()) == 0 and float(f.dww[:, 60:].abs().max()) == 0 and float(f.dwb[60:].abs().max()) == 0
    assert float(f.w2[:, 1, 48:, 4:].abs().max()) == 0, "W2 columns 60..63"
    assert torch.equal(f.dww[4, :60], sd["blocks.0.convffns.0.dwc.weight"][:, 0, 1, 1]) and f.b2.shape == (48,)
    g = packing.pack_escfp_convffn(sd, "blocks.0.proj", _lib.HAT_BF16, "cpu")
    assert (g.hid, g.hid_p) == (72, 96) and g.w1.shape == (6, 2, 64, 8) and g.w2.shape == (3, 3, 64, 8) and g.w1.dtype == torch.bfloat16
    assert float(g.w1[5].float().abs().max()) == 0 and float(g.w1[4, :, 8:16].float().abs().max()) == 0, "hidden units 72..95"
    _, sdb, _, _ = R.load_case("b")
    assert packing.pack_escfp_convffn(sdb, "blocks.1.convffns.1", _lib.HAT_F32, "cpu").hid_p == 96
    with pytest.raises(ValueError, match="not supported"):
        packing.pack_escfp_convffn(E.load_case("a")[1], "blocks.0.convffns.0", _lib.HAT_F32, "cpu")     # a 64-channel ConvFFN
    with pytest.raises(ValueError, match="not supported"):
        packing.pack_esc_convffn(sd, "blocks.0.convffns.0", _lib.HAT_F32, "cpu")                          # ... and the other way round
    assert packing.ESC_HID_PAD == {80: 96, 128: 128}


def test_large_kernel_pack():
    cfg, sd, _, _ = R.load_case("a")
    for dt, kpad in ((_lib.HAT_BF16, 2880), (_lib.HAT_F32, 2784)):
        f = packing.pack_escfp_lk(sd, "blocks.0.pconvs.0", dt, "cpu")
        assert f.kpad == kpad >= 169 * 16 and all(t.dtype == torch.float32 for t in (f.w1, f.b1, f.w2, f.b2, f.lk_channel, f.lk_spatial))
        assert f.w1.shape == (4, 16) and f.w2.shape == (144, 4) and f.lk_channel.shape == (16, 16) and f.lk_spatial.shape == (16, 169)
        assert torch.equal(f.lk_spatial[3, 13 * 2 + 5], sd["lk_spatial"][3, 0, 2, 5]) and torch.equal(f.lk_channel[3, 7], sd["lk_channel"][3, 7, 0, 0])
    with pytest.raises(ValueError, match="not supported"):
        packing.pack_escfp_lk(dict(sd, lk_spatial=torch.zeros(16, 1, 11, 11)), "blocks.0.pconvs.0", _lib.HAT_F32, "cpu")


@pytest.mark.parametrize("bad", [dict(dim=64, num_heads=4), dict(num_heads=4), dict(pdim=32), dict(kernel_size=17), dict(window_size=16),
                                 dict(exp_ratio=4)], ids=["dim64", "heads4", "pdim32", "kernel17", "window16", "exp4"])
def test_engine_refuses_shapes_that_are_not_built(bad):
    from super_resolution_amd.esc_engine import ESCFPEngine
    net = ARCH_REGISTRY.get("ESCFP")(**dict(R.CASES["a"][0], **bad))
    with pytest.raises(ValueError, match="not supported"):
        ESCFPEngine(net.cfg, net.state_dict(), "cpu", "fp32")


def test_engine_packs_on_the_host_and_esc_keeps_refusing_dim_48():
    from super_resolution_amd.esc_engine import ESCEngine, ESCFPEngine
    cfg, sd, _, _ = R.load_case("a")
    net = build_network(dict(cfg, type="ESCFP"))
    e = ESCFPEngine(net.cfg, sd, "cpu", "bf16")
    assert e.C == 48 and e.heads == 3 and e._kpad == 2880 and e.head.ptab.shape == (2, 4) and e.blocks[0].convs[0][0] is not None
    with pytest.raises(ValueError, match="compute_dtype"):
        ESCFPEngine(net.cfg, sd, "cpu", "fp16")
    with pytest.raises(ValueError, match="upscaling_factor=5"):
        n5 = build_network(dict(cfg, type="ESCFP", upscaling_factor=5))
        ESCFPEngine(n5.cfg, n5.state_dict(), "cpu", "fp32")
    esc = ARCH_REGISTRY.get("ESC")(**dict(cfg, use_ln=True))
    with pytest.raises(ValueError, match="dim=48 is not supported"):
        ESCEngine(esc.cfg, esc.state_dict(), "cpu", "fp32")


def test_refused_paths_raise_not_implemented_with_escs_message():
    net = build_network(dict(R.CASES["a"][0], type="ESCFP")).eval()
    x = torch.zeros(1, 3, 40, 40)
    for call in (lambda: net.forward_ensemble(x), lambda: net.forward_to_u8(x), lambda: net.forward_u8(x), lambda: net.forward_gt_u8(x),
                 lambda: net.forward_yuv420(x), lambda: net.forward_yuv(x), lambda: net.forward_bands(x, 2), lambda: net.forward_band_parallel(x)):
        with pytest.raises(NotImplementedError, match="runs its float forward only"):
            call()
    with pytest.raises(RuntimeError, match="GPU"):
        net(x)
    with pytest.raises(RuntimeError, match="eval"):
        net.train()(x)


def test_new_symbols_exported_and_abi_unchanged():
    with open(os.path.join(ROOT, "include", "hat_mi355x.h")) as f:
        hdr = f.read()
    assert re.search(r"#define HAT_ABI_VERSION 2\b", hdr) and _lib.ABI_VERSION == 2
    for sym in ("hat_escfp_convffn", "hat_escfp_layernorm", "hat_escfp_weights", "hat_escfp_shuffle_bicubic"):
        assert re.search(rf"\bint {sym}\(", hdr), sym
        assert sym in _lib.SIGNATURES, sym
    assert _lib.SIGNATURES["hat_escfp_convffn"] == _lib.SIGNATURES["hat_esc_convffn"]
    assert _lib.SIGNATURES["hat_escfp_layernorm"] == _lib.SIGNATURES["hat_esc_layernorm"]
    from super_resolution_amd import build
    assert "hat_escfp.hip" in build.SOURCES
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.hat_abi_version() == 2 and lib.hat_escfp_convffn(None, None) == -1
