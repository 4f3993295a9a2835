"""HybridHATNAF without a GPU: the fp64 restatement of the stem (tests/naf_ref.py) against the reference's goldens, the
pack-time folds and operand layouts against it, the module's registry name, state-dict surface, strict load and merge rules,
the argument contract of hat_naf_half / hat_naf_fold (every refusal comes before a launch), and the refusals of the engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import naf_ref as R
from helpers import golden, max_abs
from super_resolution_amd import _lib, packing
from super_resolution_amd.registry import ARCH_REGISTRY, build_network

WIDTHS = [(64, 4), (32, 2)]


@pytest.mark.parametrize("c,nb", WIDTHS)
def test_ref_matches_reference_blocks(c, nb):
    """naf_ref against the reference's own outputs on the 20x37 map: <= 1e-5, the bar the oracle is held to for HATX."""
    sd, gold = R.synth_sd(R.NAMES[c]), golden("blocks_naf.npz")
    hw = tuple(int(v) for v in gold["hw"])
    t = R.synth.normal(R.X_SEED, f"naf_in_c{c}", (1, c) + hw)
    assert max_abs(R.attn_half(t, sd, "naf.body.0")[0], gold[f"half_c{c}"]) <= 1e-5
    assert max_abs(R.block(t, sd, "naf.body.0"), gold[f"block_c{c}"]) <= 1e-5
    assert max_abs(R.stem(R.synth.synth_input(R.X_SEED, (1, 3) + hw), sd, nb), gold[f"stem_c{c}"]) <= 1e-5


@pytest.mark.parametrize("c,nb", WIDTHS)
def test_ref_matches_reference_x_naf(c, nb):
    gold = golden(f"whole_{R.NAMES[c]}.npz")
    x = R.synth.synth_input(R.X_SEED, tuple(int(v) for v in gold["x_shape"]))
    assert max_abs(R.stem(x, R.synth_sd(R.NAMES[c]), nb), gold["x_naf"]) <= 1e-5


def test_ref_zero_padding_rule_is_visible():
    """The wrong rule (u = pw1.bias outside the image) differs from the right one by O(bias) on border pixels and by nothing inside."""
    c = 32
    r, w1 = R.synth.normal(3, "r", (1, c, 5, 6)), R.synth.normal(3, "w1", (2 * c, c), std=c ** -0.5)
    b1, dw, db = torch.full((2 * c,), 0.5), torch.ones(2 * c, 1, 3, 3), torch.zeros(2 * c)
    good, bad = R.gate_half(r, w1, b1, dw, db), R.gate_half(r, w1, b1, dw, db, zero_pad_u=False)
    assert max_abs(good[:, :, 1:-1, 1:-1], bad[:, :, 1:-1, 1:-1]) == 0.0
    assert float((good - bad).abs()[:, :, 0].min()) > 0.1


def _unfrag(wf, rows, cols):
    """hat_naf_half's A fragments [rows/16][cols/32][64][8] -> the (rows, cols) matrix (the header's element order)."""
    wf = wf.float().reshape(rows // 16, cols // 32, 64, 8)
    M = torch.zeros(rows, cols)
    for lane in range(64):
        for j in range(8):
            M[(lane & 15)::16, 8 * (lane >> 4) + j::32] = wf[:, :, lane, j]
    return M


@pytest.mark.parametrize("c,nb", WIDTHS)
def test_pack_time_folds_and_layouts(c, nb):
    sd, p = R.synth_sd(R.NAMES[c]), "naf.body.1"
    blk = packing.pack_naf_block(sd, p, packing.HAT_F32, "cpu")
    assert torch.equal(_unfrag(blk.w1, 2 * c, c), sd[p + ".pw1.weight"].reshape(2 * c, c))
    assert torch.equal(_unfrag(blk.w1f, 2 * c, c), sd[p + ".ffn1.weight"].reshape(2 * c, c))
    assert torch.equal(blk.dww, sd[p + ".dw.weight"].reshape(2 * c, 9).t()) and torch.equal(blk.dwwf[4], sd[p + ".ffn_dw.weight"][:, 0, 1, 1])
    # out = y + gamma * ffn2(g2) == y + Wf2 g2 + bf2
    g2 = R.synth.normal(5, "g2", (2, c, 4, 3))
    want = sd[p + ".gamma"].double() * R.pointwise(g2, sd[p + ".ffn2.weight"], sd[p + ".ffn2.bias"])
    got = R.pointwise(g2, _unfrag(blk.wf2, c, c), blk.bf2)
    assert max_abs(got, want) <= 1e-6
    # the attention half's fold, as hat_naf_fold states it: y = x + Wf g + bf with Wf = beta * w2 * diag(s)
    g, mean = R.synth.normal(5, "g", (2, c, 4, 3)), R.synth.normal(5, "m", (2, c))
    Wf, bf = R.fold(mean, blk.wsca, blk.bsca, blk.w2, blk.b2, blk.beta)
    s = R.sca_scale(mean[:, :, None, None], sd[p + ".sca.1.weight"], sd[p + ".sca.1.bias"])
    want = sd[p + ".beta"].double() * R.pointwise(g * s[:, :, None, None], sd[p + ".pw2.weight"], sd[p + ".pw2.bias"])
    got = torch.einsum("boi,bihw->bohw", Wf, g.double()) + bf.reshape(1, -1, 1, 1)
    assert max_abs(got, want) <= 1e-12
    bb = packing.pack_naf_block(sd, p, packing.HAT_BF16, "cpu")
    assert bb.w1.dtype == torch.bfloat16 and bb.wf2.dtype == torch.bfloat16 and bb.b1.dtype == torch.float32


def _net(c, **kw):
    return build_network(dict(type="HybridHATNAF", **R.net_kwargs(R.NAMES[c]), **kw)).eval()


def test_registry_round_trip():
    from super_resolution_amd.archs.hybrid_hat_naf_arch import HybridHATNAF
    from super_resolution_amd.archs.hat_arch import HAT, HATX
    assert ARCH_REGISTRY.get("HybridHATNAF") is HybridHATNAF
    net = _net(32)
    assert isinstance(net, HybridHATNAF) and isinstance(net, HAT) and isinstance(net.hat, HATX)


@pytest.mark.parametrize("c,nb", WIDTHS)
def test_state_dict_surface_and_strict_load(c, nb):
    name = R.NAMES[c]
    net, surf = _net(c), R.surface()
    assert [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()] == surf["surfaces"][name]
    assert sum(p.numel() for p in net.parameters()) == surf["nparams"][name]
    at = surf["attrs"][name]
    assert (net.window_size, net.upscale, net.in_chans, net.img_range, net.extra_repr()) == \
        (at["window_size"], at["upscale"], at["in_chans"], at["img_range"], at["extra_repr"])
    before = net._wver
    r = net.load_state_dict(R.synth_sd(name), strict=True)
    assert not r.missing_keys and not r.unexpected_keys and net._wver > before   # the load hook saw it
    assert torch.equal(net.naf.body[0].beta, R.synth_sd(name)["naf.body.0.beta"])
    stem = {id(p) for p in net.naf.parameters()}
    assert stem and stem <= {id(p) for p in net.parameters()}            # what _weights_key walks holds the stem's parameters
    v = net._wver
    assert net.mark_weights_changed()._wver == v + 1 and net.float()._wver == v + 2     # (_apply)
    assert net.compute_dtype == "bf16" and net.set_compute_dtype("f32").compute_dtype == "f32" and _net(c, use_graph=True).use_graph


def test_merge_rules_are_the_references():
    for key, at in R.surface()["attrs"].items():
        if not key.startswith("merge:"):
            continue
        net = build_network(dict(type="HybridHATNAF", **at["kwargs"]))
        assert (net.window_size, net.upscale, net.in_chans, net.hat.window_size, net.hat.upscale) == \
            (at["window_size"], at["upscale"], at["in_chans"], at["hat_window_size"], at["hat_upscale"]), key
        assert net.cfg["window_size"] == at["hat_window_size"] and net.cfg["upscale"] == at["hat_upscale"]


def test_engine_args_are_hatx_names_plus_the_stem():
    net = _net(32)
    cfg, sd = net._engine_args()
    assert cfg["naf"] == dict(width=32, blocks=2) and cfg["variant"] == "hatx"
    assert set(sd) == set(net.hat.state_dict()) | {k for k in net.state_dict() if k.startswith("naf.")}


def test_no_cpu_path_and_band_refusal():
    net = _net(32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="SCA pool"):
        net.forward_bands(torch.rand(1, 3, 32, 16), 2)
    with pytest.raises(NotImplementedError, match="SCA pool"):
        net.forward_band_parallel(torch.rand(1, 3, 32, 16))


def test_unsupported_width_is_a_value_error_at_pack_time():
    net = build_network(dict(type="HybridHATNAF", naf_width=48, naf_blocks=1, hat_kwargs=R.net_kwargs(R.NAMES[32])["hat_kwargs"]))
    sd = {k: v for k, v in net.state_dict().items()}
    with pytest.raises(ValueError, match="naf_width 48"):
        packing.pack_naf_block(sd, "naf.body.0", packing.HAT_BF16, "cpu")
    from super_resolution_amd import engine

    class Probe(engine.HATEngine):     # the engine's own stem packer, without a device
        def __init__(self, cfg):
            self.cfg, self.dtype, self.dev = cfg, packing.HAT_BF16, "cpu"
    with pytest.raises(ValueError, match="naf_width 48"):
        Probe(net.cfg)._pack_naf(net._engine_args()[1])
    ok = _net(32)
    with pytest.raises(ValueError, match="in_chans"):
        Probe(dict(ok.cfg, in_chans=1))._pack_naf(ok._engine_args()[1])


# ---- the argument contract: every refusal below comes back before anything touches a device (there is none here)
def _half_desc(c=64, dtype=_lib.HAT_BF16, form_b=True):
    """A descriptor every check accepts, over host buffers that are never dereferenced; returns (desc, keep-alive)."""
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64
    d = _lib.HatNafHalfDesc()
    d.r_in, d.w1, d.b1, d.dww, d.dwb, d.g_out = base, base + 64, base + 128, base + 192, base + 256, base + 320
    if form_b:
        d.gprev, d.wf, d.bf, d.r_out = base + 384, base + 448, base + 512, base + 576
    d.B, d.H, d.W, d.C, d.ldr, d.ldg, d.ldo, d.dtype = 1, 8, 8, c, c, c, c, dtype
    return d, buf


def _refused(mutate, code=-1, **kw):
    d, keep = _half_desc(**kw)
    mutate(d)
    return _lib.load().hat_naf_half(C.byref(d), None) == code


def test_naf_half_argument_contract():
    lib = _lib.load()
    assert lib.hat_naf_half(None, None) == -1
    assert lib.hat_naf_half_tiles(20, 37) == 3 * 3 and lib.hat_naf_half_tiles(720, 1280) == 90 * 80 and lib.hat_naf_half_tiles(0, 5) == -1
    for c in (48, 128, 0):
        assert _refused(lambda d: setattr(d, "C", c), code=-3)            # HAT_EUNSUPPORTED: not instantiated
    for field in ("r_in", "w1", "b1", "dww", "dwb", "g_out"):
        assert _refused(lambda d: setattr(d, field, None), form_b=False), field
    for field in ("wf", "bf", "r_out", "b1", "g_out"):
        assert _refused(lambda d: setattr(d, field, None)), field
    for field, v in (("H", 0), ("W", 0), ("B", 0), ("B", 65536), ("dtype", 2), ("ldr", 63), ("ldr", 66), ("ldg", 60), ("ldg", 68), ("ldo", 68),
                     ("ldo", 56), ("wf_bstride", 4), ("wf_bstride", -8), ("bf_bstride", 2)):
        assert _refused(lambda d: setattr(d, field, v)), (field, v)
    assert _refused(lambda d: setattr(d, "r_out", d.r_in))                # form (b) writes beside what its neighbours read
    assert _refused(lambda d: setattr(d, "g_out", d.gprev))
    assert _refused(lambda d: setattr(d, "r_in", d.r_in + 4))             # misaligned
    assert _refused(lambda d: setattr(d, "gprev", d.gprev + 8))
    assert _refused(lambda d: setattr(d, "g_out", d.g_out + 2))

    def proj_with_pool(d):
        d.w1, d.partials = None, d.r_in
    assert _refused(proj_with_pool)                                       # no gated map, no pool


def test_naf_fold_argument_contract():
    lib = _lib.load()
    buf = (C.c_char * 1024)()
    base = (C.addressof(buf) + 63) // 64 * 64

    def desc():
        d = _lib.HatNafFoldDesc()
        for i, (name, _) in enumerate(_lib.HatNafFoldDesc._fields_[:8]):
            setattr(d, name, base + 64 * i)
        d.npix, d.B, d.tiles, d.C, d.dtype = 64, 1, 1, 64, _lib.HAT_F32
        return d
    assert lib.hat_naf_fold(None, None) == -1
    for name, _ in _lib.HatNafFoldDesc._fields_[:8]:
        d = desc()
        setattr(d, name, None)
        assert lib.hat_naf_fold(C.byref(d), None) == -1, name
    for field, v, code in (("B", 0, -1), ("tiles", 0, -1), ("npix", 0, -1), ("dtype", 5, -1), ("C", 48, -3), ("wf", base + 4, -1), ("bf", base + 8, -1)):
        d = desc()
        setattr(d, field, v)
        assert lib.hat_naf_fold(C.byref(d), None) == code, (field, v)


@pytest.mark.parametrize("name", ["HatNafHalfDesc", "HatNafFoldDesc"])
def test_naf_desc_layout_matches_c(tmp_path, name):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S = getattr(_lib, name)
    fields = [f[0] for f in S._fields_]
    prog = f'#include <stdio.h>\n#include <stddef.h>\n#include "hat_mi355x.h"\nint main(){{printf("%zu", sizeof({name}));\n'
    prog += "".join(f'printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + "return 0;}\n"
    (tmp_path / "layout.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(S) and vals[1:] == [getattr(S, f).offset for f in fields]
