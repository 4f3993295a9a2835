"""Host-side checks of the FP16-range guard: the option and its environment variable, the three new C entries in
the header and the binding, where the engine's plan puts guarded launches, and that the plan's function table knows none of
them.  What needs real descriptors — the entries' argument contract, embed_dim 180, a recorded plan — is tests/test_gpu_t16_guard.py's."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hat_mi355x.h")
GUARDED = {"hat_hab_tail3_guarded": "HatHabTailDesc", "hat_conv_guarded": "HatConvDesc", "hat_linear_guarded": "HatConvDesc"}


def test_option_from_env():
    from super_resolution_amd.engine import Options
    assert Options().t16_guard == "defer" and Options.from_env({}).t16_guard == "defer"
    for mode in ("defer", "sync", "off"):
        assert Options.from_env({"HAT_T16_GUARD": mode}).t16_guard == mode
    o = Options.from_env({"HAT_T16_GUARD": "sync", "HAT_NO_T16": "1", "HAT_NO_CAB_FOLD": "x"})
    assert o.no_t16 and o.no_cab_fold and not o.no_n16 and o.t16_guard == "sync"     # (the other switches read as before)
    for bad in ("1", "on", "Sync", "deferred"):
        with pytest.raises(ValueError, match="HAT_T16_GUARD"):
            Options.from_env({"HAT_T16_GUARD": bad})
    with pytest.raises(ValueError):
        Options(t16_guard="maybe")
    assert "HAT_T16_GUARD" in Options.__doc__


def test_header_and_binding_declare_the_guarded_entries():
    from super_resolution_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, desc in GUARDED.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/hat_mi355x.h"
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert args == [f"const {desc}* d", "uint32_t* sat", "void* stream"], args
        res, argt = _lib.SIGNATURES[name]
        assert res is C.c_int and argt == [C.POINTER(getattr(_lib, desc)), C.c_void_p, C.c_void_p]
        # the unguarded twin keeps its two arguments
        assert _lib.SIGNATURES[name[:-len("_guarded")]][1] == [C.POINTER(getattr(_lib, desc)), C.c_void_p]
    assert re.search(r"#define\s+HAT_ABI_VERSION\s+2\b", open(HEADER).read()) and _lib.ABI_VERSION == 2


def test_guarded_entries_take_a_null_descriptor():
    """(what the entries refuse on descriptors that would launch is tests/test_gpu_t16_guard.py's: it needs a device)"""
    from super_resolution_amd import _lib
    lib = _lib.load()
    word = (C.c_uint32 * 2)()
    for name in GUARDED:
        assert getattr(lib, name)(None, C.addressof(word), None) == -1
    assert word[0] == 0


def _plan(t16, mode, depths=(2, 3), conv_after_body=True, tails="fused144"):
    """HATEngine's stream plan on a packed network reduced to what _plan_t16 reads: no weights, no device."""
    from super_resolution_amd.engine import HATEngine, _Group, _Hab, _Ocab
    eng = HATEngine.__new__(HATEngine)
    eng.t16, eng.t16_guard = t16, mode
    eng.conv_after_body = object() if conv_after_body else None
    eng.layers = []
    for depth in depths:
        habs = []
        for _ in range(depth):
            hb = _Hab()
            hb.tail, hb.ffn3 = tails, types.SimpleNamespace(C=144)
            habs.append(hb)
        oc = _Ocab()
        oc.mlpf, oc.proj = object(), types.SimpleNamespace(frag=True, nt=9)
        G = _Group(6, habs, oc, types.SimpleNamespace(frag=False, ksize=3, nt=9, n_slices=1, nout=144))
        G.to_conv, G.conv_ln = True, ((None, None), 16)
        eng.layers.append(G)
    eng._plan_t16()
    return eng


def test_plan_guards_exactly_the_fp16_stores():
    eng = _plan(True, "defer")
    want = []
    for gi, G in enumerate(eng.layers):
        want += [("tail", gi, i) for i, hb in enumerate(G.habs) if hb.out16] + ([("proj", gi)] if G.ocab16 else []) + ([("conv", gi)] if G.out16 else [])
    assert eng.guarded_launches() == want
    # HAT-S shaped groups: every tail, every projection and every group conv hands FP16 rows on
    assert want == [("tail", 0, 0), ("tail", 0, 1), ("proj", 0), ("conv", 0), ("tail", 1, 0), ("tail", 1, 1), ("tail", 1, 2), ("proj", 1), ("conv", 1)]
    assert _plan(True, "sync").guarded_launches() == want
    assert _plan(True, "off").guarded_launches() == []
    # no FP16 stream (HAT_NO_T16=1, embed_dim 180, fp32: t16 is False for all three): no FP16 store, no guarded launch
    off = _plan(False, "defer")
    assert off.guarded_launches() == [] and not any(hb.out16 for G in off.layers for hb in G.habs) and not any(G.out16 or G.ocab16 for G in off.layers)
    # a tail that is not the 144 one reads fp32, so whatever feeds one stores fp32 and is not guarded; what is left is the last
    # group's conv, whose FP16 rows nobody reads (the network goes on from its fused LayerNorm rows)
    assert _plan(True, "defer", tails="fused180").guarded_launches() == [("conv", 1)]
    # a fallback re-plans: what was FP16 is fp32 again
    eng.t16 = False
    eng._plan_t16()
    assert eng.guarded_launches() == [] and not any(hb.out16 for G in eng.layers for hb in G.habs)


def test_plans_know_no_guarded_entry():
    """The plan's function table (and the loader's mirror of it) has no guarded entry, and the recorder keeps only calls of that
    table: a guarded call would pass through unrecorded.  (A recorded forward's call list: tests/test_gpu_t16_guard.py.)"""
    from super_resolution_amd import plan
    assert not any(n.endswith("_guarded") for n in plan.FN_IDS)
    parse = open(os.path.join(ROOT, "super_resolution_amd", "csrc", "hat_plan_parse.h")).read()
    assert "_guarded" not in parse
    rec = plan._Recorder(types.SimpleNamespace(hat_conv_guarded=lambda *a: 0, hat_conv=lambda *a: 0))
    rec.hat_conv_guarded(1, 2, 3)
    rec.hat_conv(1, 2)
    assert [n for n, _ in rec.calls] == ["hat_conv"]
