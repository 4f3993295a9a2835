"""ESC without a GPU: the fp64 restatement (tests/esc_ref.py) against the reference's goldens, the state-dict surface, the registry,
the constructor refusals, the harness' model types, the exported symbols and the reflect-gather identity the attention kernel uses."""
import os
import re

import numpy as np
import pytest
import torch

import esc_ref
from super_resolution_amd import _lib, packing
from super_resolution_amd.registry import ARCH_REGISTRY, build_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_taps(t, px):
    return t[0].reshape(64, -1)[:, px].t()


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_reference_goldens(name):
    cfg, sd, g, _ = esc_ref.load_case(name)
    taps = {}
    y = esc_ref.forward(esc_ref.d64(sd), cfg, torch.from_numpy(g["x"]).double(), taps)
    assert float((y - torch.from_numpy(g["y"]).double()).abs().max()) <= 1e-5
    px = torch.from_numpy(g["tap_pixels"])
    for k in esc_ref.TAPS:
        assert float((_flat_taps(taps[k], px) - torch.from_numpy(g[k]).double()).abs().max()) <= 1e-5, k


def test_restatement_converted_and_rescaled():
    cfg, sd, g, meta = esc_ref.load_case("c")
    sd64 = esc_ref.d64(sd)
    sd64["plk_filter"] = esc_ref.geo_ensemble(sd64["plk_filter"])
    y = esc_ref.forward(sd64, cfg, torch.from_numpy(g["x"]).double(), converted=True)
    assert float((y - torch.from_numpy(g["y"]).double()).abs().max()) <= 1e-5
    assert meta["converted_max_abs_vs_a"] <= 1e-5   # the reference's own converted output equals its unconverted one
    cfg, sd, g, _ = esc_ref.load_case("d")
    sd64 = esc_ref.d64(sd)
    sd64["to_img.weight"], sd64["to_img.bias"] = esc_ref.convert_to_img(sd64["to_img.weight"], sd64["to_img.bias"], 3)
    y = esc_ref.forward(sd64, cfg, torch.from_numpy(g["x"]).double())
    assert y.shape == (1, 3, 99, 120)
    assert float((y - torch.from_numpy(g["y"]).double()).abs().max()) <= 1e-5


def test_state_dict_surface_matches_reference():
    meta = esc_ref.surfaces()
    for name, ent in list(meta["surfaces"].items()) + [(k, meta["cases"][k]) for k in "ab"]:
        net = build_network(dict(ent["cfg"], type="ESC", attn_type="Naive"))
        got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert got == ent["surface"], name
    assert meta["cases"]["a"]["nparams"] == 193368 and len(meta["cases"]["a"]["surface"]) == 38


def test_registry_round_trip_and_load():
    ESC = ARCH_REGISTRY.get("ESC")
    cfg, sd, _, _ = esc_ref.load_case("a")
    net = ESC(**cfg)
    assert net.upscaling_factor == 2 and net.window_size == 32 and net.compute_dtype == "bf16" and not net.use_graph
    net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(NotImplementedError):
        ESC(**cfg, attn_type="Other")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        net.eval()(torch.zeros(1, 3, 40, 40))
    with pytest.raises(RuntimeError, match="eval"):
        net.train()(torch.zeros(1, 3, 40, 40))
    for what in (lambda: net.forward_ensemble(None), lambda: net.forward_u8(None), lambda: net.forward_yuv(None, fmt="nv12"),
                 lambda: net.forward_bands(None, 2), lambda: net.forward_band_parallel(None)):
        with pytest.raises(NotImplementedError):
            what()


def test_convert_bakes_the_geo_ensemble():
    cfg, sd, _, _ = esc_ref.load_case("a")
    net = ARCH_REGISTRY.get("ESC")(**cfg)
    net.load_state_dict(sd)
    net.convert()
    assert torch.equal(net.plk_filter.detach(), packing.esc_geo_ensemble(sd["plk_filter"]))
    assert net.cfg["converted"] and list(net.state_dict()) == list(sd)
    net.convert()   # idempotent
    assert torch.equal(net.plk_filter.detach(), packing.esc_geo_ensemble(sd["plk_filter"]))


def test_load_state_dict_converts_to_img_between_scales():
    cfg, sd, _, _ = esc_ref.load_case("a")
    net = ARCH_REGISTRY.get("ESC")(**dict(cfg, upscaling_factor=3))
    net.load_state_dict(sd, strict=True)
    k, b = esc_ref.convert_to_img(sd["to_img.weight"], sd["to_img.bias"], 3)
    assert net.to_img.weight.shape == (27, 64, 3, 3)
    assert torch.equal(net.to_img.weight.detach(), k) and torch.equal(net.to_img.bias.detach(), b)
    assert sd["to_img.weight"].shape == (12, 64, 3, 3)   # the caller's dict is left as it was


@pytest.mark.parametrize("bad", [dict(dim=192, window_size=48), dict(pdim=32), dict(kernel_size=17), dict(num_heads=8), dict(exp_ratio=4),
                                 dict(window_size=16)])
def test_engine_refuses_shapes_that_are_not_built(bad):
    from super_resolution_amd.esc_engine import ESCEngine
    cfg = dict(esc_ref.CASES["a"][0], **bad)
    net = ARCH_REGISTRY.get("ESC")(**cfg)
    with pytest.raises(ValueError, match="not supported"):
        ESCEngine(net.cfg, net.state_dict(), "cpu", "fp32")


def test_convffn_packing_layout():
    cfg, sd, _, _ = esc_ref.load_case("a")
    f = packing.pack_esc_convffn(sd, "blocks.0.convffns.0", _lib.HAT_F32, "cpu")
    assert (f.hid, f.hid_p) == (80, 96) and f.w1.shape == (6, 2, 64, 8) and f.w2.shape == (4, 3, 64, 8) and f.dww.shape == (9, 96)
    W1, W2 = sd["blocks.0.convffns.0.proj.weight"].reshape(80, 64), sd["blocks.0.convffns.0.aggr.weight"].reshape(64, 80)
    t, ks, lane, j = 3, 1, 37, 5
    assert f.w1[t, ks, lane, j] == W1[16 * t + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
    assert f.w2[t, ks, lane, j] == W2[16 * t + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
    assert float(f.w1[5].abs().max()) == 0 and float(f.b1[80:].abs().max()) == 0 and float(f.dww[:, 80:].abs().max()) == 0
    assert torch.equal(f.dww[4, :80], sd["blocks.0.convffns.0.dwc.weight"][:, 0, 1, 1])
    assert packing.pack_esc_convffn(sd, "blocks.0.proj", _lib.HAT_F32, "cpu").hid_p == 128


def test_esr_model_resolves():
    from super_resolution_amd import models
    assert models.model_class("ESRModel") is models.HATModel and models.model_class("HATModel") is models.HATModel
    assert models.model_class(None) is models.HATModel
    with pytest.raises(KeyError):
        models.model_class("SwinIRModel")


def test_new_symbols_exported_and_abi_unchanged():
    with open(os.path.join(ROOT, "include", "hat_mi355x.h")) as f:
        hdr = f.read()
    assert re.search(r"#define HAT_ABI_VERSION 2\b", hdr) and _lib.ABI_VERSION == 2
    for sym in ("hat_esc_convffn", "hat_esc_convffn_tiles", "hat_window_attention_r", "hat_esc_layernorm", "hat_esc_shuffle_add"):
        assert re.search(rf"\bint {sym}\(", hdr), sym
        assert sym in _lib.SIGNATURES, sym
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.hat_abi_version() == 2
        assert lib.hat_esc_convffn_tiles(20, 37) == 3 * 4 and lib.hat_esc_convffn_tiles(0, 5) == _lib_einval()


def _lib_einval():
    return -1


@pytest.mark.parametrize("hw", [(40, 72), (33, 64)])
def test_reflect_gather_identity(hw):
    """to_qkv is a 1x1 conv, so padding then projecting equals projecting then gathering from the reflected coordinates: exactly."""
    cfg, sd, _, _ = esc_ref.load_case("a")
    sd64 = esc_ref.d64(sd)
    x = esc_ref.synth.normal(7, f"gather{hw}", (1, 64) + hw).double()
    a = esc_ref.window_attention(x, sd64, "blocks.0.attn", 32, 4, gather=False)
    b = esc_ref.window_attention(x, sd64, "blocks.0.attn", 32, 4, gather=True)
    assert torch.equal(a, b)
    assert np.array_equal(esc_ref.reflect_index(33, 64).numpy()[33:], np.arange(31, 0, -1))


def test_reflect_pad_and_logits_of_the_restatement():
    """What test_gpu_esc_edges.py adds to esc_ref: reflect_pad is F.pad(mode="reflect") at the smallest legal frame and at the largest
    pad, and the logits attention_core hands back are the ones its output is the softmax of (a per-head shift leaves it unchanged)."""
    F = torch.nn.functional
    for h, w in [(17, 17), (33, 65), (32, 32)]:
        x = esc_ref.synth.normal(7, f"pad{h}x{w}", (2, 5, h, w)).double()
        assert torch.equal(esc_ref.reflect_pad(x, 32), F.pad(x, (0, (-w) % 32, 0, (-h) % 32), mode="reflect"))
    qkv = esc_ref.synth.normal(7, "logit_qkv", (1, 96, 32, 32)).double()
    table = esc_ref.synth.normal(7, "logit_rpb", (2, 63 * 63), std=0.5).double()
    o, s = esc_ref.attention_core(qkv, table, 32, 2, logits=True)
    assert s.shape == (1, 2, 1024, 1024) and torch.equal(o, esc_ref.attention_core(qkv, table, 32, 2))
    v = qkv[0, 64:].reshape(2, 16, 1024).transpose(1, 2)
    assert float((torch.softmax(s[0], -1) @ v - o[0].reshape(2, 16, 1024).transpose(1, 2)).abs().max()) == 0.0
    shifted = esc_ref.attention_core(qkv, table + torch.tensor([[100.0], [-100.0]], dtype=torch.float64), 32, 2)
    assert float((shifted - o).abs().max()) <= 1e-12
