"""ESCRealM without a GPU: the constructor and the state_dict surface against the reference's (escrealm_surface.json), MetaUpsample,
the fp64 restatement (tests/escrealm_ref.py) against the reference's goldens, the reference's error messages, the pack-time
refusals, the pack-time folds, and the argument contract of the new C entries (refused before any device call)."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import escrealm_ref as R
from helpers import max_abs, rnd

KW = dict(R.BASE, n_blocks=1, conv_blocks=1, upscaling_factor=2)


def _build(**kw):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    return build_network(dict(type="ESCRealM", **kw))


def test_constructor_signature_is_the_references():
    from super_resolution_amd.archs.esc_real_m_arch import ESCRealM
    p = list(inspect.signature(ESCRealM.__init__).parameters.values())[1:]
    assert [a.name for a in p] == ["dim", "pdim", "kernel_size", "n_blocks", "conv_blocks", "window_size", "num_heads", "upscaling_factor", "exp_ratio",
                                   "attn_type", "mid_dim", "upsampler", "unshuffle_mod", "compute_dtype", "use_graph"]
    assert {a.name: a.default for a in p if a.default is not inspect.Parameter.empty} == dict(
        exp_ratio=2, attn_type="Flex", mid_dim=48, upsampler="nearest+conv", unshuffle_mod=True, compute_dtype="bf16", use_graph=False)


@pytest.mark.parametrize("name", list(R.CASES) + list(R.SURFACE_CFGS))
def test_surface_key_for_key(name):
    meta = R.surfaces()
    ent = meta["cases"][name] if name in R.CASES else meta["surfaces"][name]
    net = _build(**ent["cfg"])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == ent["surface"]
    mu = net.state_dict()["to_img.MetaUpsample"]
    assert mu.dtype == torch.uint8 and mu.tolist() == ent["meta_upsample"] == R.meta_upsample(ent["cfg"])
    assert sum(p.numel() for p in net.parameters()) == (ent["nparams"] if name in R.CASES else meta["nparams"][name])


def test_stem_keys_and_block_layernorms():
    un, plain = _build(**KW).state_dict(), _build(**dict(KW, unshuffle_mod=False)).state_dict()
    assert tuple(un["proj.1.weight"].shape) == (64, 12, 3, 3) and tuple(un["skip.1.weight"].shape) == (128, 12, 1, 1)
    assert {"skip.2.weight", "skip.4.weight"} <= set(un) and "proj.weight" not in un
    assert tuple(plain["proj.weight"].shape) == (64, 3, 3, 3) and {"skip.0.weight", "skip.1.weight", "skip.3.weight"} <= set(plain)
    assert "blocks.0.lns.0.weight" in un   # the reference's Block always carries its per-conv-block LayerNorms
    assert tuple(_build(**dict(KW, upscaling_factor=1)).state_dict()["proj.1.weight"].shape) == (64, 48, 3, 3)
    assert _build(**KW).upscale == 2 and _build(**dict(KW, upscaling_factor=4, upsampler="conv")).upscale == 1


def test_load_state_dict_ignores_the_checkpoints_metaupsample():
    net = _build(**KW)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["to_img.MetaUpsample"] = torch.tensor([9, 9, 9, 9, 9, 9, 9], dtype=torch.uint8)
    net.load_state_dict(sd, strict=True)
    assert net.to_img.MetaUpsample.tolist() == [2, 3, 4, 64, 3, 48, 4]
    del sd["to_img.MetaUpsample"]
    net.load_state_dict(sd, strict=True)   # and a checkpoint without one loads
    assert not hasattr(type(net), "convert") or pytest.raises(AttributeError, lambda: net.convert)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference(name):
    cfg, sd, g, meta = R.load_case(name)
    taps = {}
    y = R.forward(R.d64(sd), cfg, torch.from_numpy(g["x"]).double(), taps)
    assert list(y.shape) == meta["out"] and list(taps["feat"].shape[-2:]) == meta["body"]
    assert max_abs(y, g["y"]) <= 1e-5
    if name in R.TAP_CASES:
        px = torch.from_numpy(g["tap_pixels"])
        assert max_abs(R.rows_at(taps["skip"], px), g["skip"]) <= 1e-5 and max_abs(R.rows_at(taps["feat"], px), g["feat"]) <= 1e-5


def test_the_references_error_messages():
    with pytest.raises(NotImplementedError, match="Attention type Fast is not supported."):
        _build(**dict(KW, attn_type="Fast"))
    with pytest.raises(ValueError, match="An invalid Upsample was selected. Please choose one of typing.Literal"):
        _build(**dict(KW, upsampler="bilinear"))
    for up in ("pixelshuffle", "nearest+conv"):
        with pytest.raises(ValueError, match="scale 5 is not supported. Supported scales: 2\\^n and 3."):
            _build(**dict(KW, upscaling_factor=5, upsampler=up))


def test_pack_time_refusals():
    pack = lambda **kw: _build(**dict(KW, **kw))._make_engine("cpu")
    pack()
    with pytest.raises(ValueError, match="multiple of 16"):
        pack(upsampler="pixelshuffle", mid_dim=40)
    with pytest.raises(ValueError, match="mid_dim 48 and 64"):
        pack(upsampler="dysample", mid_dim=32)
    with pytest.raises(ValueError, match="upscaling_factor=8"):
        pack(upscaling_factor=8, upsampler="pixelshuffledirect")
    with pytest.raises(ValueError, match="unshuffled stem"):
        pack(upsampler="conv")
    with pytest.raises(ValueError, match="dim=48"):
        pack(dim=48)
    eng = pack()
    with pytest.raises(RuntimeError, match="at least 4"):
        eng._check_frame(3, 20)
    assert eng._body_size(67, 81) == (34, 41) and pack(upscaling_factor=1)._body_size(66, 83) == (17, 21) and pack(upscaling_factor=3)._body_size(33, 40) == (33, 40)
    for fn in ("forward_ensemble", "forward_to_u8", "forward_u8", "forward_yuv420", "forward_yuv"):
        with pytest.raises(NotImplementedError):
            getattr(_build(**KW), fn)(None)


@pytest.mark.parametrize("r", [2, 3])
def test_conv_nearest_fold_is_exact(r):
    from super_resolution_amd import packing
    w, b, x = rnd("cnw", (8, 5, 3, 3)).double(), rnd("cnb", (8,)).double(), rnd("cnx", (1, 5, 7, 9)).double()
    wf, bf = packing.conv_nearest_fold(w, b, r)
    want = F.interpolate(F.conv2d(x, w, b, padding=1), scale_factor=r, mode="nearest")
    assert torch.equal(F.pixel_shuffle(F.conv2d(x, wf, bf, padding=1), r), want)
    perm = packing.pixshuf_perm(8 * r * r, r)   # packed row ij * 8 + c holds channel c r^2 + ij
    assert perm.tolist() == [c * r * r + ij for ij in range(r * r) for c in range(8)]


def test_new_entries_refuse_bad_arguments_without_a_device():
    """Every refusal below is decided from the arguments alone: no GPU is needed, and none is touched."""
    from super_resolution_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert p % 16 == 0 or True
    a = (p + 15) // 16 * 16
    skip = lambda **kw: lib.hat_escrealm_skip(*dict(dict(x=a, w0=a, b0=a, dw=a, bdw=a, w3=a, b3=a, r=None, out=a + 64, B=1, H=8, W=8, cin=12, ldx=12,
                                                         ldr=64, ldo=64, dtype=0), **kw).values(), None)
    for kw in [dict(x=None), dict(b0=None), dict(bdw=None), dict(b3=None), dict(out=None), dict(out=a), dict(x=a + 4), dict(w3=a + 8), dict(ldx=8),
               dict(ldo=66), dict(ldo=60), dict(r=a + 4), dict(r=a, ldr=60), dict(H=3), dict(W=0), dict(B=0), dict(B=65536), dict(dtype=2)]:
        assert skip(**kw) == -1, kw
    assert skip(cin=3) == -3 and skip(cin=24, ldx=24) == -3
    un = lambda x=a, rows=a + 64, B=1, h=5, w=7, f=2, ld=12: lib.hat_unshuffle_pad(x, rows, B, h, w, f, ld, None)
    assert un(x=None) == un(rows=None) == un(rows=a) == un(B=0) == un(h=0) == un(ld=8) == un(f=4, ld=44) == un(f=4, h=1, ld=48) == -1
    assert un(f=3, ld=27) == un(f=1) == un(f=8, ld=192) == -3
    sh = lambda rows=a, y=a + 64, B=1, H=3, W=4, s=2, ld=12: lib.hat_shuffle_planes(rows, y, B, H, W, s, ld, None)
    assert sh(rows=None) == sh(y=None) == sh(y=a) == sh(W=0) == sh(s=0) == sh(s=9, ld=243) == sh(ld=8) == sh(s=3, ld=24) == -1
