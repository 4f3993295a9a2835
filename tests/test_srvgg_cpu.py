"""SRVGGNetCompact off the device: the fp64 restatement against the reference's goldens (tests/golden/srvgg_*.npz,
gen_golden_srvgg.py), the class's state-dict surface, the registry, the refusals, pack_vgg_conv as a pure relayout with its digest
pinned, HatVggConvDesc's C layout, hat_vgg_conv's argument checks (they precede every launch, so they run without a GPU), the
harness on the fixture option file, and the domain conditions of the exact-lattice cases test_gpu_srvgg.py launches."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import pytest
import torch

import srvgg_lattice as VL
import srvgg_ref as R
from helpers import max_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_OPT = os.path.join(R.GOLDEN, "srvgg_x4_toy.yml")


@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


# ---- the restatement and the surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference(name):
    cfg, sd, g, meta = R.load_case(name)
    assert (cfg, meta["frame"]) == (R.CASES[name][0], list(R.CASES[name][1]))
    x = torch.from_numpy(g["x"])
    assert torch.equal(x, R.case_input(name))
    taps = {}
    y = R.forward(R.d64(sd), cfg, x.double(), taps=taps)
    assert list(y.shape) == meta["out"]
    assert max_abs(y, g["y"]) <= 1e-5 and max_abs(y - R.nearest(x.double(), cfg["upscale"]), g["res"]) <= 1e-5
    assert float(torch.from_numpy(g["res"]).std()) >= 0.1
    if name == R.TAP_CASE:
        assert max_abs(R.rows_at(taps[R.TAP_LAYER], g["tap_pixels"]), g["tap"]) <= 1e-5
        assert g["tap"].shape == (R.N_TAP_PIXELS, 64) and (g["tap_pixels"] == R.tap_pixels(*x.shape[2:])).all()


def _surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def test_state_dict_surface_is_the_reference_s():
    import super_resolution_amd.archs  # noqa: F401
    from super_resolution_amd.registry import ARCH_REGISTRY, build_network
    meta = R.surfaces()
    assert "SRVGGNetCompact" in ARCH_REGISTRY
    for name, case in list(meta["cases"].items()) + list(meta["surfaces"].items()):
        net = build_network(dict(case["cfg"], type="SRVGGNetCompact"))
        assert _surface(net) == case["surface"] == R.surface_of(case["cfg"]), name
        assert sum(p.numel() for p in net.parameters()) == case["nparams"]
        assert net.upscale == case["cfg"]["upscale"]
    assert len(meta["surfaces"]["x4_16"]["surface"]) == 18 * 2 + 17 and len(meta["surfaces"]["x4_32"]["surface"]) == 34 * 2 + 33
    relu = build_network(dict(R.CASES["c"][0], type="SRVGGNetCompact"))
    assert not any(k.endswith(".weight") and v.dim() == 1 for k, v in relu.state_dict().items())   # no activation contributes a key
    cfg, sd, _, _ = R.load_case("e")
    net = build_network(dict(cfg, type="SRVGGNetCompact", compute_dtype="fp32", use_graph=True)).eval()
    net.load_state_dict(sd, strict=True)
    assert net.use_graph and all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())


def test_refusals():
    from super_resolution_amd.archs.srvgg_arch import SRVGGNetCompact
    from super_resolution_amd.srvgg_engine import SRVGGEngine
    with pytest.raises(ValueError, match="act_type"):
        SRVGGNetCompact(act_type="gelu")
    for bad in (dict(num_feat=32), dict(num_in_ch=1), dict(num_out_ch=1), dict(upscale=5), dict(num_in_ch=4, num_out_ch=4)):
        net = SRVGGNetCompact(**dict(dict(num_conv=1), **bad)).eval()
        with pytest.raises(ValueError, match="built for num_feat 64"):
            net.engine("cpu")
    with pytest.raises(ValueError, match="compute_dtype"):
        SRVGGNetCompact(num_conv=0, compute_dtype="fp8").eval().engine("cpu")
    net = SRVGGNetCompact(num_conv=1).eval()
    eng = net.engine("cpu")     # a host device is taken: the engine packs and never runs
    assert isinstance(eng, SRVGGEngine) and len(eng.layers) == 2 and eng._pad_multiple() == 1 and eng.ld == 48
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x)
    with pytest.raises(RuntimeError, match="eval"):
        SRVGGNetCompact(num_conv=0)(x)
    for call in (lambda: net.forward_bands(x, 2), lambda: net.forward_band_parallel(x)):
        with pytest.raises(NotImplementedError, match="row-band"):
            call()
    for call, word in ((lambda: net.forward_u8(x), "upscale_u8"), (lambda: net.forward_gt_u8(x), "upscale_gt_u8"), (lambda: net.forward_to_u8(x), "upscale_to_u8"),
                       (lambda: net.forward_yuv(x), "upscale_yuv"), (lambda: net.forward_yuv420(x), "upscale_yuv"), (lambda: net.forward_ensemble(x), "upscale_ensemble")):
        with pytest.raises(NotImplementedError, match="SRVGGNetCompact runs .*" + word):     # the network's own name, and the call to use
            call()
    from super_resolution_amd import plan
    with pytest.raises(NotImplementedError, match="cannot be exported"):
        plan.record_plan(net, (1, 3, 8, 8))


# ---- packing ------------------------------------------------------------------------------------------------------------------
def _wt(*shape, k=1):
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.int64) * 2654435761 * k) % 1021 - 510).float() / 256).reshape(shape)


def _unpack(pv, dtype):
    """The weight tensor back from hat_vgg_conv's image, by the layout the header states: [slice][k-step][n-tile][lane][j] holds
    output 16 (slice ntl + n-tile) + lane % 16, k = 32 k-step + 8 (lane / 16) + j; rows: k = 64 tap + ci; frame: k = 9 ci + tap."""
    from super_resolution_amd import packing
    ntl = packing.VGG_NTL[dtype]
    nsl, ks = 4 // ntl, (1 if pv.frame else 18)
    assert tuple(pv.w.shape) == (nsl, ks, ntl, 64, 8)
    sl, kk, nt, lane, j = torch.meshgrid(torch.arange(nsl), torch.arange(ks), torch.arange(ntl), torch.arange(64), torch.arange(8), indexing="ij")
    n, k = 16 * (sl * ntl + nt) + lane % 16, 32 * kk + 8 * (lane // 16) + j
    m = torch.zeros(64, 32 * ks, dtype=pv.w.dtype)
    m[n.reshape(-1), k.reshape(-1)] = pv.w.reshape(-1)
    if pv.frame:
        assert not m[:, 27:].any()
        return m[:, :27].reshape(64, 3, 3, 3)
    return m.reshape(64, 3, 3, 64).permute(0, 3, 1, 2)


def _digest(pv):
    h = hashlib.sha256()
    for t in (pv.w, pv.bias, pv.slope):
        h.update(str((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_pack_vgg_conv_is_a_relayout_with_a_pinned_digest():
    from super_resolution_amd import ops
    with open(os.path.join(R.GOLDEN, "srvgg_packing_digests.json")) as f:
        pinned = json.load(f)["cases"]
    got = {}
    for dname, dt in (("bf16", ops.HAT_BF16), ("f32", ops.HAT_F32)):
        for cin in (64, 3):
            w, b, s = _wt(64, cin, 3, 3), _wt(64, k=3), _wt(64, k=7)
            pv = ops.pack_vgg_conv(w, b, s, dt, "cpu")
            assert pv.frame == (cin == 3) and pv.w.dtype == ops.TORCH_DTYPE[dt] and pv.w.is_contiguous()
            assert torch.equal(_unpack(pv, dt), w.to(ops.TORCH_DTYPE[dt])), (dname, cin)     # (the one rounding to T, nothing else)
            assert torch.equal(pv.bias, b) and torch.equal(pv.slope, s) and pv.bias.dtype == pv.slope.dtype == torch.float32
            got[f"{dname}_{cin}"] = _digest(pv)
    assert got == pinned
    with pytest.raises(ValueError, match="built for"):
        ops.pack_vgg_conv(_wt(64, 32, 3, 3), _wt(64), _wt(64), ops.HAT_BF16, "cpu")
    with pytest.raises(ValueError, match="built for"):
        ops.pack_vgg_conv(_wt(64, 64, 3, 3), _wt(64), _wt(1), ops.HAT_BF16, "cpu")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_vgg_desc_layout_matches_c(lib, tmp_path):
    """Compile a tiny C program against the header and compare sizeof / offsetof with ctypes (test_cabi_cpu.py's method)."""
    from super_resolution_amd import _lib
    S = _lib.HatVggConvDesc
    fields = [f[0] for f in S._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hat_mi355x.h"\nint main(){printf("%zu", sizeof(HatVggConvDesc));\n'
    prog += "".join(f'printf(" %zu", offsetof(HatVggConvDesc, {f}));\n' for f in fields) + "return 0;}\n"
    (tmp_path / "layout.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(S) and vals[1:] == [getattr(S, f).offset for f in fields]
    assert lib.hat_abi_version() == 2


def test_vgg_conv_rejects_bad_arguments_without_gpu(lib):
    """Every refusal precedes the first HIP call, so made-up (aligned, non-null) addresses do: nothing is dereferenced."""
    from super_resolution_amd import _lib
    good = dict(x=0x10000, w=0x20000, bias=0x30000, slope=0x40000, out=0x50000, B=1, H=8, W=8, ldx=64, ldo=64, frame=0, dtype=_lib.HAT_BF16)

    def call(**kw):
        d = _lib.HatVggConvDesc()
        for k, v in dict(good, **kw).items():
            setattr(d, k, v)
        return lib.hat_vgg_conv(C.byref(d), None)

    bad = [dict(x=None), dict(w=None), dict(bias=None), dict(slope=None), dict(out=None),                                  # null pointers
           dict(x=0x10008), dict(w=0x20008), dict(bias=0x30004), dict(slope=0x40008), dict(out=0x50002), dict(x=0x10002, frame=1),   # misaligned
           dict(B=0), dict(H=0), dict(W=0), dict(B=-1),
           dict(ldo=63), dict(ldo=68), dict(ldx=56), dict(ldx=68), dict(ldo=66, dtype=_lib.HAT_F32), dict(ldx=66, dtype=_lib.HAT_F32),   # leading dimensions
           dict(out=0x10000), dict(dtype=2), dict(dtype=-1),
           dict(B=65536, H=16 * 256, W=16 * 256), dict(B=4097, H=16 * 512, W=16 * 512)]                                     # 2^32 tiles; 2^30 + 2^18: past the limit of 2^30
    for kw in bad:
        assert call(**kw) == -1, f"{kw}: expected HAT_EINVAL"
    assert lib.hat_vgg_conv(None, None) == -1
    t, g, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    q = lambda *a: lib.hat_vgg_conv_tiles(*a, C.byref(t), C.byref(g), C.byref(s))
    assert q(1, 0, 8, _lib.HAT_BF16) == -1 and q(1, 8, 8, 5) == -1 and lib.hat_vgg_conv_tiles(1, 8, 8, 1, None, C.byref(g), C.byref(s)) == -1
    assert q(4097, 16 * 512, 16 * 512, _lib.HAT_BF16) == -1 and q(4096, 16 * 512, 16 * 512, _lib.HAT_BF16) == 0 and t.value == 1 << 30
    assert q(1, 720, 1280, _lib.HAT_BF16) == 0 and (t.value, g.value, s.value) == (45 * 80, 256, 1)
    assert q(1, 720, 1280, _lib.HAT_F32) == 0 and (t.value, g.value, s.value) == (45 * 80, 128, 2)
    assert q(2, 33, 40, _lib.HAT_BF16) == 0 and (t.value, g.value, s.value) == (18, 24, 1)      # no idle group of eight on a small frame
    assert q(1, 1, 1, _lib.HAT_F32) == 0 and (t.value, g.value, s.value) == (1, 8, 2)


def test_resident_convs_share_one_schedule(lib):
    """conv3_groups (csrc/hat_conv3_tile.h) through its two queries and the Python restatement the conv64r tests use: the same
    workgroups per slice for the same (slices, tiles), whole groups of eight, at most 256 workgroups in all, no idle group."""
    from lattice import conv64r_trip_tiles
    from super_resolution_amd import ops
    queries = {1: [lambda g: ops.vgg_conv_tiles(*g, ops.HAT_BF16), lambda g: ops.rdb_conv_tiles(*g, 64)],
               2: [lambda g: ops.vgg_conv_tiles(*g, ops.HAT_F32), lambda g: ops.rdb_conv_tiles(*g, 192)]}
    for tiles in list(range(1, 301)) + [2047, 2048, 2049, (1 << 20) + 1, (1 << 30) - 1, 1 << 30]:
        geoms = [(tiles, 1, 1)] + ([(1, 1, 16 * tiles)] if tiles <= 300 else [])
        for nsl, qs in queries.items():
            got = {q(g) for q in qs for g in geoms}
            wgs = conv64r_trip_tiles(nsl, tiles)[0]
            assert got == {(tiles, wgs, nsl)}, (tiles, nsl, got, wgs)
            assert wgs % 8 == 0 and wgs <= 256 // nsl and (wgs <= 8 or wgs - 8 < tiles), (tiles, nsl, wgs)


# ---- the harness --------------------------------------------------------------------------------------------------------------
def test_harness_parses_the_fixture_option_file():
    import yaml
    from super_resolution_amd.models import MODEL_TYPES, HATModel, model_class
    from super_resolution_amd.test import parse_options
    assert model_class("SRModel") is HATModel and model_class("RealESRNetModel") is HATModel and MODEL_TYPES["HATModel"] is HATModel
    opt = parse_options(FIXTURE_OPT, u8=True)
    assert opt["model_type"] == "SRModel" and opt["network_g"]["type"] == "SRVGGNetCompact" and "window_size" not in opt["network_g"]
    assert opt["val"]["u8_on_device"] and opt["datasets"]["test_1"]["phase"] == "test" and opt["datasets"]["test_1"]["scale"] == 4
    with open(FIXTURE_OPT) as f:
        raw = yaml.safe_load(f)
    assert {k: v for k, v in raw["network_g"].items() if k != "type"} == R.SURFACE_CFGS["x4_16"]
    m = HATModel.__new__(HATModel)      # the one helper that reads window_size: the key's value where it is there, else 1
    m.opt = opt
    assert m._window_size() == 1
    m.opt = {"network_g": {"window_size": 16}}
    assert m._window_size() == 16


# ---- the lattice cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_lattice_cases_are_inside_the_exact_domain(lib, dtype):
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    big = VL.two_trip_geom(lambda B, H, W: ops.vgg_conv_tiles(B, H, W, dt))
    tiles, wgs, nsl = ops.vgg_conv_tiles(*big, dt)
    assert big == (1, 1, 16 * wgs + 1) and wgs == 256 // nsl and sorted(set(VL.trips(tiles, wgs))) == [1, 2]
    assert VL.trips(tiles, wgs).count(2) == 1
    for geom in VL.GEOMS + [big]:
        for mode in VL.MODES:
            c = VL.vgg_case(geom, mode, dtype)
            assert c.ref.shape == geom + (64,)
