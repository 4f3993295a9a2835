"""RRDBNet off the device: the fp64 restatement against the reference's goldens (tests/golden/rrdb_*.npz, gen_golden_rrdb.py), the
class's state-dict surface, the registry and the harness's model types, the refusals, pack_rdb_conv as a pure relayout with its
digest pinned, HatRdbConvDesc's C layout, hat_rdb_conv's argument checks (they precede every launch, so they run without a GPU),
hat_unshuffle_pad's channel order against pixel_unshuffle, and the domain conditions of the exact-lattice cases test_gpu_rrdb.py
launches."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import escrealm_ref
import rrdb_lattice as RL
import rrdb_ref as R
from helpers import max_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_OPT = os.path.join(R.GOLDEN, "rrdb_x4_toy.yml")


@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


# ---- the restatement and the surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.CASES if n != "d"] + ["d"])
def test_restatement_matches_the_reference(name):
    cfg, sd, g, meta = R.load_case(name)
    assert (cfg, meta["frame"], meta["gain"]) == (R.CASES[name][0], list(R.CASES[name][1]), R.CASES[name][2])
    x = torch.from_numpy(g["x"])
    assert torch.equal(x, R.case_input(name))
    taps = {}
    y = R.forward(R.d64(sd), cfg, x.double(), taps=taps)
    assert list(y.shape) == meta["out"] and max_abs(y, g["y"]) <= 1e-5
    assert 0.1 <= float(torch.from_numpy(g["y"]).std()) <= 1.0 and meta["bf16"]["psnr"] >= 40.0
    if name == R.TAP_CASE:
        assert max_abs(R.rows_at(taps[R.TAP_BLOCK], g["tap_pixels"]), g["tap"]) <= 1e-5
        assert g["tap"].shape == (R.N_TAP_PIXELS, 64) and (g["tap_pixels"] == R.tap_pixels(*x.shape[2:])).all()


def _surface(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


def test_state_dict_surface_is_the_reference_s():
    import super_resolution_amd.archs  # noqa: F401
    from super_resolution_amd.registry import ARCH_REGISTRY, build_network
    meta = R.surfaces()
    assert "RRDBNet" in ARCH_REGISTRY
    for name, case in list(meta["cases"].items()) + list(meta["surfaces"].items()):
        net = build_network(dict(case["cfg"], type="RRDBNet"))
        assert _surface(net) == case["surface"] == R.surface_of(case["cfg"]), name
        assert sum(p.numel() for p in net.parameters()) == case["nparams"]
        assert net.scale == net.upscale == case["cfg"]["scale"]
    assert len(meta["surfaces"]["x4_23"]["surface"]) == 2 * (23 * 15 + 6) and meta["surfaces"]["x2_23"]["surface"][0][1] == [64, 12, 3, 3]
    assert meta["surfaces"]["x4_23"]["nparams"] == 16697987       # RealESRGAN_x4plus / ESRGAN
    from super_resolution_amd.archs.rrdbnet_arch import RRDBNet
    net = RRDBNet(3, 3)                                            # the reference's positional signature and defaults
    assert net.cfg == R.SURFACE_CFGS["x4_23"] and net.compute_dtype == "bf16" and not net.use_graph
    cfg, sd, _, _ = R.load_case("e")
    net = build_network(dict(cfg, type="RRDBNet", compute_dtype="fp32", use_graph=True)).eval()
    net.load_state_dict(sd, strict=True)
    assert net.use_graph and all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())


def test_model_types_and_the_fixture_option_file():
    import yaml
    from super_resolution_amd.models import MODEL_TYPES, HATModel, model_class
    from super_resolution_amd.test import parse_options
    for t in ("ESRGANModel", "SRGANModel", "RealESRGANModel", "SRModel", "HATModel"):
        assert model_class(t) is HATModel and MODEL_TYPES[t] is HATModel
    with pytest.raises(KeyError, match="not built"):
        model_class("VideoRecurrentModel")
    opt = parse_options(FIXTURE_OPT, u8=True)
    assert opt["model_type"] == "RealESRGANModel" and opt["network_g"]["type"] == "RRDBNet" and "window_size" not in opt["network_g"]
    with open(FIXTURE_OPT) as f:
        raw = yaml.safe_load(f)
    assert {k: v for k, v in raw["network_g"].items() if k != "type"} == R.CASES["a"][0]
    m = HATModel.__new__(HATModel)      # the multiple the harness pads to: the unshuffle factor
    for s, want in ((4, 1), (2, 2), (1, 4)):
        m.opt = {"network_g": dict(raw["network_g"], scale=s)}
        assert m._window_size() == want


def test_refusals():
    from super_resolution_amd.archs.rrdbnet_arch import RRDBNet
    from super_resolution_amd.rrdb_engine import RRDBEngine
    for bad in (dict(scale=3), dict(scale=8), dict(num_feat=32), dict(num_grow_ch=16), dict(num_in_ch=1), dict(num_out_ch=1)):
        net = RRDBNet(**dict(dict(num_in_ch=3, num_out_ch=3, num_block=1), **bad)).eval()
        with pytest.raises(ValueError, match="built for num_feat 64, num_grow_ch 32"):
            net.engine("cpu")
    with pytest.raises(ValueError, match="compute_dtype"):
        RRDBNet(3, 3, num_block=0, compute_dtype="fp8").eval().engine("cpu")
    net = RRDBNet(3, 3, scale=2, num_block=1).eval()
    eng = net.engine("cpu")     # a host device is taken: the engine packs and never runs
    assert isinstance(eng, RRDBEngine) and len(eng.blocks) == 1 and [len(r) for r in eng.blocks[0]] == [5, 5, 5]
    assert eng._pad_multiple() == 2 and eng._out_factor() == 2 and eng._body_size(38, 34) == (19, 17)
    assert RRDBNet(3, 3, scale=1, num_block=0).eval().engine("cpu")._pad_multiple() == 4 and RRDBNet(3, 3, num_block=0).eval().engine("cpu")._pad_multiple() == 1
    with pytest.raises(AssertionError, match="37x34"):      # an odd frame at scale 2: the reference's refusal, naming the size
        eng._check_input(torch.zeros(1, 3, 37, 34))
    eng._check_input(torch.zeros(2, 3, 38, 34))
    with pytest.raises(RuntimeError, match=r"\(B,3,h,w\)"):
        eng._check_input(torch.zeros(1, 4, 8, 8))
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x)
    with pytest.raises(RuntimeError, match="eval"):
        RRDBNet(3, 3, num_block=0)(x)
    for call in (lambda: net.forward_bands(x, 2), lambda: net.forward_band_parallel(x)):
        with pytest.raises(NotImplementedError, match="row-band"):
            call()
    for call, word in ((lambda: net.forward_u8(x), "upscale_u8"), (lambda: net.forward_yuv(x), "upscale_yuv"), (lambda: net.forward_ensemble(x), "upscale_ensemble")):
        with pytest.raises(NotImplementedError, match="RRDBNet runs .*" + word):
            call()
    from super_resolution_amd import plan
    with pytest.raises(NotImplementedError, match="cannot be exported"):
        plan.record_plan(net, (1, 3, 8, 8))


def test_unshuffle_pad_channel_order_is_pixel_unshuffle_s():
    """hat_unshuffle_pad is pinned to escrealm_ref.unshuffle_pad on the device (test_gpu_escrealm.py); on a frame that f divides that
    restatement, this file's own, and torch's pixel_unshuffle (what arch_util.py:186-203 computes) are one function."""
    for f, (h, w) in ((2, (38, 34)), (4, (20, 36))):
        x = torch.arange(2 * 3 * h * w, dtype=torch.float32).reshape(2, 3, h, w)
        assert torch.equal(escrealm_ref.unshuffle_pad(x, f), F.pixel_unshuffle(x, f)) and torch.equal(R.unshuffle(x, f), F.pixel_unshuffle(x, f))


# ---- packing ------------------------------------------------------------------------------------------------------------------
def _wt(*shape, k=1):
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.int64) * 2654435761 * k) % 1021 - 510).float() / 256).reshape(shape)


def _unpack(pr):
    """The weight tensor back from hat_rdb_conv's image, by the layout the header states: [slice][k-step][n-tile][lane][j] holds output
    32 slice + 16 n-tile + lane % 16, k-step = 9 (channel / 32) + tap, channel % 32 = 8 (lane / 16) + j."""
    nsl, ks = pr.cout // 32, 9 * pr.cin // 32
    assert tuple(pr.w.shape) == (nsl, ks, 2, 64, 8)
    sl, kk, nt, lane, j = torch.meshgrid(torch.arange(nsl), torch.arange(ks), torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    n, ch, tap = 32 * sl + 16 * nt + lane % 16, 32 * (kk // 9) + 8 * (lane // 16) + j, kk % 9
    w = torch.zeros(pr.cout, pr.cin, 9, dtype=pr.w.dtype)
    w[n.reshape(-1), ch.reshape(-1), tap.reshape(-1)] = pr.w.reshape(-1)
    return w.reshape(pr.cout, pr.cin, 3, 3)


def _digest(pr):
    h = hashlib.sha256()
    for t in (pr.w, pr.bias):
        h.update(str((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_pack_rdb_conv_is_a_relayout_with_a_pinned_digest():
    from super_resolution_amd import ops
    with open(os.path.join(R.GOLDEN, "rrdb_packing_digests.json")) as f:
        pinned = json.load(f)["cases"]
    got = {}
    assert ops.RDB_CIN == RL.CINS
    for cin in ops.RDB_CIN:
        cout = 64 if cin == 192 else 32
        w, b = _wt(cout, cin, 3, 3), _wt(cout, k=3)
        pr = ops.pack_rdb_conv(w, b, ops.HAT_BF16, "cpu")
        assert (pr.cin, pr.cout) == (cin, cout) and pr.w.dtype == torch.bfloat16 and pr.w.is_contiguous()
        assert pr.w.numel() * 2 == (36864, 55296, 73728, 92160, 221184)[ops.RDB_CIN.index(cin)]      # the header's byte counts
        assert torch.equal(_unpack(pr), w.to(torch.bfloat16)), cin     # (the one rounding to T, nothing else)
        assert torch.equal(pr.bias, b) and pr.bias.dtype == torch.float32
        got[f"bf16_{cin}"] = _digest(pr)
    assert got == pinned
    for shape, bshape in (((32, 80, 3, 3), (32,)), ((64, 64, 3, 3), (64,)), ((32, 192, 3, 3), (32,)), ((32, 64, 1, 1), (32,)), ((32, 64, 3, 3), (64,))):
        with pytest.raises(ValueError, match="built for"):
            ops.pack_rdb_conv(_wt(*shape), _wt(*bshape), ops.HAT_BF16, "cpu")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_rdb_desc_layout_matches_c(lib, tmp_path):
    """Compile a tiny C program against the header and compare sizeof / offsetof with ctypes (test_cabi_cpu.py's method)."""
    from super_resolution_amd import _lib
    S = _lib.HatRdbConvDesc
    fields = [f[0] for f in S._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hat_mi355x.h"\nint main(){printf("%zu", sizeof(HatRdbConvDesc));\n'
    prog += "".join(f'printf(" %zu", offsetof(HatRdbConvDesc, {f}));\n' for f in fields) + "return 0;}\n"
    (tmp_path / "layout.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(S) and vals[1:] == [getattr(S, f).offset for f in fields]
    assert lib.hat_abi_version() == 2


def test_rdb_conv_rejects_bad_arguments_without_gpu(lib):
    """Every refusal precedes the first HIP call, so made-up (aligned, non-null) addresses do: nothing is dereferenced."""
    from super_resolution_amd import _lib
    good = dict(x=0x10000, w=0x20000, bias=0x30000, out=0x10000, B=1, H=8, W=8, cin=96, cout=32, ldx=192, ldo=192, out_off=96,
                slope=0.2, beta1=1.0, beta2=1.0, dtype=_lib.HAT_BF16)
    last = dict(good, out=0x50000, cin=192, cout=64, out_off=0, r1=0x60000, r2=0x70000, s_out=0x80000)

    def call(base, **kw):
        d = _lib.HatRdbConvDesc()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.hat_rdb_conv(C.byref(d), None)

    bad = [dict(x=None), dict(w=None), dict(bias=None), dict(out=None),                                          # null pointers
           dict(x=0x10008, out=0x50000), dict(w=0x20008), dict(bias=0x30004), dict(out=0x50002),                 # misaligned
           dict(cin=80), dict(cin=32), dict(cin=224), dict(cin=0), dict(cout=64), dict(cout=16), dict(cin=192),   # cin; cout against cin
           dict(ldx=88), dict(ldx=196), dict(ldo=120), dict(ldo=196, out=0x50000), dict(out_off=100), dict(out_off=-8), dict(out_off=168),   # leading dimensions
           dict(out_off=64), dict(ldo=200),                                                                      # in place: a slot that is read; another pitch
           dict(B=0), dict(H=0), dict(W=0), dict(B=-1),
           dict(r1=0x60000), dict(s_out=0x80000),                                                                # the fp32 stream belongs to conv 5
           dict(dtype=2), dict(dtype=-1),
           dict(B=65536, H=16 * 256, W=16 * 256), dict(B=4097, H=16 * 512, W=16 * 512)]                           # 2^32 tiles; past 2^30
    for kw in bad:
        assert call(good, **kw) == -1, f"{kw}: expected HAT_EINVAL"
    bad5 = [dict(s_out=None), dict(r1=None), dict(r1=0x60004), dict(r2=0x70008), dict(s_out=0x80004), dict(cout=32), dict(ldo=56), dict(ldx=184)]
    for kw in bad5:                                                                                              # (r1=None: r2 without r1)
        assert call(last, **kw) == -1, f"conv 5 {kw}: expected HAT_EINVAL"
    assert lib.hat_rdb_conv(None, None) == -1
    # the fp32 instantiation does not exist: the checks pass, then HAT_EUNSUPPORTED, before any launch
    assert call(good, dtype=_lib.HAT_F32) == -3 and call(last, dtype=_lib.HAT_F32) == -3 and call(last, r2=None, r1=None, dtype=_lib.HAT_F32) == -3
    assert call(good, dtype=_lib.HAT_F32, ldx=194, ldo=194) == -1        # (fp32 rows: whole 16 bytes are 4 elements)
    t, g, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    q = lambda *a: lib.hat_rdb_conv_tiles(*a, C.byref(t), C.byref(g), C.byref(s))
    assert q(1, 0, 8, 64) == -1 and q(1, 8, 8, 80) == -1 and lib.hat_rdb_conv_tiles(1, 8, 8, 64, None, C.byref(g), C.byref(s)) == -1
    assert q(4097, 16 * 512, 16 * 512, 64) == -1 and q(4096, 16 * 512, 16 * 512, 64) == 0 and t.value == 1 << 30
    assert q(1, 720, 1280, 160) == 0 and (t.value, g.value, s.value) == (45 * 80, 256, 1)
    assert q(1, 720, 1280, 192) == 0 and (t.value, g.value, s.value) == (45 * 80, 128, 2)
    assert q(2, 33, 40, 64) == 0 and (t.value, g.value, s.value) == (18, 24, 1)      # no idle group of eight on a small frame
    assert q(1, 1, 1, 192) == 0 and (t.value, g.value, s.value) == (1, 8, 2)


# ---- the lattice cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", RL.CINS)
def test_lattice_cases_are_inside_the_exact_domain(lib, cin):
    from super_resolution_amd import ops
    big = RL.two_trip_geom(lambda B, H, W: ops.rdb_conv_tiles(B, H, W, cin))
    tiles, wgs, nsl = ops.rdb_conv_tiles(*big, cin)
    assert big == (1, 1, 16 * wgs + 1) and wgs == 256 // nsl and sorted(set(RL.trips(tiles, wgs))) == [1, 2]
    used = set()
    for gi, geom in enumerate(RL.GEOMS + [big]):
        used.update(RL.params(cin, gi))
        for form in RL.FORMS[cin]:
            c = RL.rdb_case(geom, cin, form)      # (raises outside the domain)
            assert c.ref.shape == geom + (c.cout,) and (c.r2 is not None) == (form == "r1r2")
    assert used <= set(RL.POW2) and len(used) >= 8
    assert {v for c_ in RL.CINS for gi in range(7) for v in RL.params(c_, gi)} == set(RL.POW2)
