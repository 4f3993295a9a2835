"""The ESC family's frame paths without a GPU: the symbol, signature and argument contract of hat_shuffle_to_u8 / hat_shuffle_to_yuv,
the ops wrappers' refusals, the `upscale_*` surface of ESC, ESCReal, ESCRealM and ESCFP beside the `forward_*` names that keep raising,
frames.upscale_frames' dispatch (with stub networks), and FrameBoundary's two hooks on HATEngine."""
import ctypes as C

import numpy as np
import pytest
import torch

import esc_ref
import escfp_ref
import escreal_ref
import escrealm_ref
import test_cabi_cpu
from super_resolution_amd import _lib
from super_resolution_amd.registry import build_network

EINVAL, EUNSUPPORTED = -1, -3   # HAT_EINVAL, HAT_EUNSUPPORTED (include/hat_mi355x.h)
HEAD = [C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 4   # rows, ld, base, B, H, W, s


def test_symbols_and_signatures():
    names = test_cabi_cpu.header_functions()
    assert "hat_shuffle_to_u8" in names and "hat_shuffle_to_yuv" in names
    assert _lib.SIGNATURES["hat_shuffle_to_u8"] == (C.c_int, HEAD + [C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 3 + [C.c_void_p])
    assert _lib.SIGNATURES["hat_shuffle_to_yuv"] == (C.c_int, HEAD + [C.POINTER(_lib.HatYuvSurface), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert lib.hat_shuffle_to_u8.argtypes == _lib.SIGNATURES["hat_shuffle_to_u8"][1]
    assert lib.hat_shuffle_to_yuv.argtypes == _lib.SIGNATURES["hat_shuffle_to_yuv"][1]


A = 1 << 20   # a non-null, 4-byte aligned address: every refusal below happens before any launch or dereference


def _u8(**kw):
    a = dict(rows=A, ld=12, base=A + 4096, B=1, H=5, W=7, s=2, dst=A + 8192, pitch=3 * 14, bstride=0, h_out=10, w_out=14, bgr=0)
    a.update(kw)
    return _lib.load().hat_shuffle_to_u8(*a.values(), None)


def test_hat_shuffle_to_u8_refuses_bad_arguments_without_a_device():
    for bad in (dict(rows=None), dict(dst=None), dict(rows=A + 2), dict(base=A + 1), dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(s=0),
                dict(ld=11), dict(h_out=0), dict(w_out=0), dict(h_out=11), dict(w_out=15), dict(pitch=41), dict(w_out=13, pitch=38),
                dict(B=2, bstride=9 * 42 + 41), dict(H=50000, W=50000), dict(s=8, ld=192, H=9000, h_out=65536, w_out=1, pitch=3)):
        assert _u8(**bad) == EINVAL, bad
    assert _u8(s=9, ld=243) == EUNSUPPORTED


def _surf(h, w, fmt="i420", depth=8, **kw):
    bps = 1 if depth == 8 else 2
    sx, sy = {"i420": (1, 1), "i422": (1, 0), "i444": (0, 0)}.get(fmt, (0, 0))
    s = _lib.HatYuvSurface(y=A + 8192, y_pitch=bps * w, y_bstride=bps * w * h, depth=depth, msb=0)
    if fmt != "gray":
        s.cb, s.cr, s.c_pitch, s.c_step, s.c_bstride, s.sub_x, s.sub_y = A + 16384, A + 20480, bps * (w >> sx), bps, bps * (w >> sx) * (h >> sy), sx, sy
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _yuv(surf, null_dst=False, null_m=False, **kw):
    a = dict(rows=A, ld=12, base=None, B=1, H=5, W=7, s=2)
    crop = dict(h_out=10, w_out=14)
    for k in list(kw):
        (crop if k in crop else a)[k] = kw.pop(k)
    m = (C.c_float * 12)(*([0.0] * 12))
    return _lib.load().hat_shuffle_to_yuv(*a.values(), None if null_dst else C.byref(surf), crop["h_out"], crop["w_out"], None if null_m else m, None)


def test_hat_shuffle_to_yuv_refuses_bad_arguments_without_a_device():
    ok = _surf(10, 14)
    assert _yuv(ok, null_dst=True) == EINVAL and _yuv(ok, null_m=True) == EINVAL
    for bad in (dict(rows=None), dict(rows=A + 1), dict(s=0), dict(ld=11), dict(h_out=12), dict(w_out=16), dict(B=0)):
        assert _yuv(ok, **bad) == EINVAL, bad
    assert _yuv(ok, s=9, ld=243) == EUNSUPPORTED
    # odd crops on the subsampled axes, whatever the surface was sized for
    assert _yuv(_surf(9, 14), h_out=9) == EINVAL and _yuv(_surf(10, 13), w_out=13) == EINVAL
    assert _yuv(_surf(10, 13, "i422"), w_out=13) == EINVAL
    # short pitches, a null plane, one chroma pointer without the other, odd pitches of words, an unknown depth
    for bad in (dict(y_pitch=13), dict(c_pitch=6), dict(y=None), dict(cr=None), dict(c_step=3), dict(depth=9), dict(msb=2)):
        assert _yuv(_surf(10, 14, **bad)) == EINVAL, bad
    assert _yuv(_surf(10, 14, depth=10, y_pitch=29)) == EINVAL and _yuv(_surf(10, 14, depth=10, y=A + 8193)) == EINVAL
    assert _yuv(_surf(10, 14, y_bstride=139), B=2) == EINVAL and _yuv(_surf(10, 14, c_bstride=34), B=2) == EINVAL   # overlapping samples


def test_ops_wrappers_refuse_wrong_dtypes_and_shapes():
    """The wrappers check before they touch the library's launch path: host tensors are refused with the other mistakes."""
    from super_resolution_amd import ops
    rows, base = torch.zeros(1, 35, 12), torch.zeros(1, 3, 5, 7)
    dst = torch.zeros(1, 10, 14, 3, dtype=torch.uint8)
    geo = dict(B=1, H=5, W=7, s=2, ld=12)
    with pytest.raises(RuntimeError, match="device rows"):
        ops.shuffle_to_u8(rows, base, dst, **geo)
    with pytest.raises(RuntimeError, match="shuffle factor"):
        ops.shuffle_to_u8(rows, base, dst, **dict(geo, s=9))
    with pytest.raises(RuntimeError, match="shuffle factor"):
        ops.shuffle_to_yuv(rows, None, dst[..., 0], None, None, [0.0] * 12, sub=None, **dict(geo, s=0))
    with pytest.raises(RuntimeError, match="device rows"):
        ops.shuffle_to_u8(rows.double(), base, dst, **geo)
    with pytest.raises(RuntimeError, match="device rows"):
        ops.shuffle_to_yuv(rows, None, dst[..., 0], None, None, [0.0] * 12, sub=None, **dict(geo, ld=11))


CASES = [("ESC", esc_ref, "a"), ("ESCReal", escreal_ref, "b"), ("ESCRealM", escrealm_ref, "a"), ("ESCFP", escfp_ref, "c")]


@pytest.mark.parametrize("arch,ref,name", CASES, ids=[c[0] for c in CASES])
def test_modules_have_upscale_calls_and_forward_names_keep_raising(arch, ref, name):
    net = build_network(dict(ref.CASES[name][0], type=arch)).eval()
    assert net.arbitrary_scale is False
    for fn in ("upscale_u8", "upscale_gt_u8", "upscale_to_u8", "upscale_yuv", "upscale_ensemble"):
        assert callable(getattr(net, fn)), fn
    x = torch.zeros(1, 3, 40, 40)
    for fn in ("forward_ensemble", "forward_to_u8", "forward_u8", "forward_gt_u8", "forward_yuv420", "forward_yuv"):
        with pytest.raises(NotImplementedError, match="upscale_"):
            getattr(net, fn)(x)
    u8 = torch.zeros(20, 24, 3, dtype=torch.uint8)
    for call in (lambda: net.upscale_u8(u8), lambda: net.upscale_gt_u8(u8), lambda: net.upscale_to_u8(x), lambda: net.upscale_ensemble(x),
                 lambda: net.upscale_yuv(torch.zeros(30, 24, dtype=torch.uint8), fmt="i420")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        net.upscale_ensemble(x, 3)
    with pytest.raises(TypeError, match="uint8 tensor"):
        net.upscale_yuv(torch.zeros(30, 24), fmt="i420")
    with pytest.raises(RuntimeError, match="eval"):
        net.train().upscale_u8(u8)


def test_esclte_is_marked_and_keeps_its_own_calls():
    import inspect
    from super_resolution_amd.registry import ARCH_REGISTRY
    lte = ARCH_REGISTRY.get("ESCLTE")
    assert lte.arbitrary_scale is True
    assert "size" in inspect.signature(lte.upscale_u8).parameters and "size" in inspect.signature(lte.upscale_yuv).parameters
    assert not hasattr(lte, "upscale_to_u8") and not hasattr(lte, "upscale_ensemble")
    net = build_network(dict(type="ESCLTE", n_blocks=1, conv_blocks=1)).eval()
    for fn in ("forward_ensemble", "forward_u8", "forward_yuv"):   # its refusals name no call it does not have
        with pytest.raises(NotImplementedError, match="runs its float forward only") as e:
            getattr(net, fn)(None)
        assert "upscale_ensemble" not in str(e.value) and "upscale_gt_u8" not in str(e.value)


def test_engines_take_the_frame_boundary_and_esclte_refuses_it():
    from super_resolution_amd.esc_engine import ESCEngine, ESCFPEngine, ESCLTEEngine, ESCRealEngine, ESCRealMEngine
    from super_resolution_amd.frame_boundary import FrameBoundary
    for cls in (ESCEngine, ESCRealEngine, ESCRealMEngine, ESCFPEngine, ESCLTEEngine):
        assert issubclass(cls, FrameBoundary)
    factors = {}
    for arch, ref, name in CASES + [("ESCReal", escreal_ref, "c"), ("ESCRealM", escrealm_ref, "b")]:
        net = build_network(dict(ref.CASES[name][0], type=arch, compute_dtype="fp32")).eval()
        eng = net._make_engine(torch.device("cpu"))   # (a host device: the engine packs and never runs)
        assert eng.cfg["in_chans"] == 3 and eng._pad_multiple() == 1
        assert (eng.u8_fused_calls, eng.u8_planes_calls, eng.yuv_fused_calls, eng.yuv_planes_calls) == (0, 0, 0, 0)
        assert eng._out_factor() == net.upscale, (arch, name)
        factors[(arch, name)] = (eng._out_factor(), int(net.cfg["upscaling_factor"]))
        with pytest.raises(RuntimeError, match="one frame" if arch != "ESCFP" else "reflect-padded"):
            eng._check_input(torch.zeros(2, 3, 16, 24))
    assert factors[("ESCReal", "b")] == (4, 2), "ESCReal's default head is x4 whatever upscaling_factor says"
    lte = build_network(dict(type="ESCLTE", n_blocks=1, conv_blocks=1, compute_dtype="fp32")).eval()._make_engine(torch.device("cpu"))
    for fn in ("forward_ensemble", "forward_to_u8", "forward_u8", "forward_gt_u8", "forward_yuv420", "forward_yuv"):
        with pytest.raises(RuntimeError, match="query_grid_u8 / query_grid_yuv"):
            getattr(lte, fn)(None)


def test_hooks_leave_hat_as_it_was():
    from super_resolution_amd.engine import HATEngine
    from super_resolution_amd.frame_boundary import FrameBoundary
    assert HATEngine._pad_multiple is FrameBoundary._pad_multiple and HATEngine._out_factor is FrameBoundary._out_factor
    eng = HATEngine.__new__(HATEngine)   # (HATEngine packs on a GPU only; the hooks read two attributes)
    eng.ws, eng.scale = 8, 3
    assert eng._pad_multiple() == 8 and eng._out_factor() == 3


# ---- frames.upscale_frames' dispatch ------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """What upscale_frames asks of a network before the device: parameters, `upscale`, and the calls it picks between.  On a host
    device the generator stops at 'needs the network on a GPU', after the dispatch decisions that raise."""
    upscale = 2

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


class _FixedStub(_Stub):
    arbitrary_scale = False

    def upscale_u8(self, *a, **k):
        raise AssertionError("not reached on a host device")

    upscale_yuv = upscale_u8


class _ArbStub(_FixedStub):
    arbitrary_scale = True


def test_upscale_frames_dispatch_with_stub_networks():
    from super_resolution_amd import frames
    rgb = [np.zeros((20, 24, 3), np.uint8)]
    # a stub fixed-scale network of the family without size= goes through upscale_u8 / upscale_yuv, the 4:2:0 layouts too
    assert frames.entry_points(_FixedStub()) == ("upscale_u8", "upscale_yuv", None)
    assert frames.fixed_scale_family(_FixedStub()) and not frames.fixed_scale_family(_ArbStub()) and not frames.fixed_scale_family(_Stub())
    # a network that has no upscale_u8 stays on HAT's names; one marked arbitrary-scale behaves as before: without size= it is sent to
    # the fixed-scale names (which ESCLTE refuses), with size= to its upscale_* calls
    assert frames.entry_points(_Stub()) == ("forward_u8", "forward_yuv", "forward_yuv420")
    assert frames.entry_points(_ArbStub()) == ("forward_u8", "forward_yuv", "forward_yuv420")
    assert frames.entry_points(_ArbStub(), arb=True) == ("upscale_u8", "upscale_yuv", None)
    # size= / scale=: only a network marked arbitrary-scale, in the words used before
    for net in (_FixedStub(), _Stub()):
        with pytest.raises(RuntimeError, match=f"size= / scale= need an arbitrary-scale network .* {type(net).__name__} has a fixed scale"):
            next(frames.upscale_frames(net, rgb, size=(30, 36)))
    with pytest.raises(ValueError, match="exactly one"):
        next(frames.upscale_frames(_ArbStub(), rgb, size=(30, 36), scale=1.5))
    with pytest.raises(RuntimeError, match="ensemble"):
        next(frames.upscale_frames(_ArbStub(), rgb, size=(30, 36), ensemble=2))
    for net, kw in ((_ArbStub(), dict(size=(30, 36))), (_FixedStub(), {}), (_FixedStub(), dict(ensemble=4))):
        with pytest.raises(RuntimeError, match="on a GPU"):   # (past every dispatch decision: the stubs live on the host)
            next(frames.upscale_frames(net, rgb, **kw))
    # the real modules
    assert frames.entry_points(build_network(dict(escreal_ref.CASES["b"][0], type="ESCReal"))) == ("upscale_u8", "upscale_yuv", None)
    lte = build_network(dict(type="ESCLTE", n_blocks=1, conv_blocks=1))
    assert frames.entry_points(lte, arb=True) == ("upscale_u8", "upscale_yuv", None) and frames.entry_points(lte)[0] == "forward_u8"
