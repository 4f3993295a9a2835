"""The fp64 restatements that tests/test_gpu_hatx_ops.py compares the kernels with (helpers.ref_keybias, ref_attention_kb,
ref_sgfn_gate) pinned to oracle/hat_oracle.py — itself validated against the reference's goldens (test_hatx_oracle.py) — and the
argument contract of hat_ocab_keybias / hat_ocab_attention_kb / hat_sgfn_gate / hat_add_f32 (every check returns before a launch,
so it runs without a GPU, as test_cabi_cpu.py's does)."""
import ctypes as C

import pytest
import torch

from oracle import hat_oracle as O
from super_resolution_amd import synth
from helpers import max_abs, ref_attention_kb, ref_keybias, ref_sgfn_gate

TOL = 1e-12
WINDOWS = [(16, 24), (8, 12), (16, 25), (8, 13)]
OVERLAP = {24: 0.5, 12: 0.5, 25: 0.6, 13: 0.7}


def _inputs(ws, wse, heads=2, d=4, B=2):
    """3 x 4 windows: interior windows, all four edges, all four corners."""
    H, W, Cc = 3 * ws, 4 * ws, heads * d
    n = lambda key, shape, std=1.0: synth.normal(5, f"{key}{wse}", shape, std=std).double()
    return dict(q=n("q", (B, H, W, Cc)) * d ** -0.5, k=n("k", (B, H, W, Cc)), v=n("v", (B, H, W, Cc)), sal=n("s", (B, H, W), 2.0),
                table=n("t", ((ws + wse - 1) ** 2, heads), 0.5), rpi=O.rpi_oca(ws, OVERLAP[wse]), heads=heads)


@pytest.mark.parametrize("ratio", [0.6, 1.0])
@pytest.mark.parametrize("mode", ["focus", "norm"])
@pytest.mark.parametrize("ws,wse", WINDOWS)
def test_keybias_then_attention_is_the_oracles_hatx_attention(ws, wse, mode, ratio):
    i = _inputs(ws, wse)
    assert ws + int(ws * OVERLAP[wse]) == wse
    nk, pad = wse * wse, (wse - ws + 1) // 2
    sal = i["sal"] if mode == "focus" else None
    k_keep = max(1, int(ratio * nk)) if ratio < 1.0 else nk
    kb, keep = ref_keybias(sal, i["k"], ws, wse, pad, k_keep)
    assert kb.shape == (2, 3, 4, (nk + 15) // 16 * 16) and keep.shape == (2, 3, 4, nk)
    assert (keep.sum(-1) == k_keep).all() and (torch.isneginf(kb[..., :nk]) == ~keep).all() and (kb[..., nk:] == 0).all()
    if mode == "norm":
        assert (kb[..., :nk][keep] == 0).all()
    got = ref_attention_kb(i["q"], i["k"], i["v"], i["table"], i["rpi"], ws, wse, i["heads"], kb)
    ref = O.hatx_ocab_attention(i["q"], i["k"], i["v"], i["table"], i["rpi"], ws, wse, i["heads"], 1.0, sal, ratio, tie="lowest_index")
    assert max_abs(got, ref) <= TOL


def test_keybias_breaks_ties_by_the_lowest_key_index():
    """A constant map: every in-image key ties, the zero-padded ones tie below them; a stable descending sort keeps the first."""
    ws, wse, pad = 8, 13, 3
    sal = torch.full((1, 24, 24), 0.5, dtype=torch.float64)
    kb, keep = ref_keybias(sal, None, ws, wse, pad, 50)
    assert keep[0, 1, 1].tolist() == [j < 50 for j in range(169)]          # interior window: no padded key
    corner = keep[0, 0, 0].reshape(13, 13)                                  # rows / columns 0..2 are outside the image
    assert not corner[:3].any() and not corner[:, :3].any() and int(corner.sum()) == 50 and corner[3:8, 3:].all()
    assert (kb[0, 1, 1, :50] == torch.tanh(torch.tensor(0.5, dtype=torch.float64))).all() and (kb[..., 169:] == 0).all()


@pytest.mark.parametrize("ws,wse", WINDOWS)
def test_attention_with_a_zero_key_bias_is_the_plain_attention(ws, wse):
    i = _inputs(ws, wse)
    kb = torch.zeros(2, 3, 4, (wse * wse + 15) // 16 * 16, dtype=torch.float64)
    kb[..., wse * wse:] = float("nan")                                      # (the dead tail is not read)
    got = ref_attention_kb(i["q"], i["k"], i["v"], i["table"], i["rpi"], ws, wse, i["heads"], kb)
    attn = O.hatx_ocab_attention if wse % 2 else O.ocab_attention
    assert max_abs(got, attn(i["q"], i["k"], i["v"], i["table"], i["rpi"], ws, wse, i["heads"], 1.0)) <= TOL


@pytest.mark.parametrize("half,geom", [(36, (2, 19, 23)), (12, (1, 3, 5)), (8, (1, 1, 7))])
def test_sgfn_gate_then_fc2_is_the_oracles_sgfn(half, geom):
    B, H, W = geom
    Cc = half  # (mlp_ratio 2: fc1 doubles the width, the gate keeps it, fc2 folds it back)
    n = lambda key, shape, std=1.0: synth.normal(6, f"{key}{half}", shape, std=std).double()
    sd = {"m.fc1.weight": n("w1", (2 * half, Cc), Cc ** -0.5), "m.fc1.bias": n("b1", (2 * half,), 0.1),
          "m.dw.weight": n("wd", (half, 1, 3, 3), 1 / 3), "m.dw.bias": n("bd", (half,), 0.1),
          "m.fc2.weight": n("w2", (Cc, 2 * half), (2 * half) ** -0.5), "m.fc2.bias": n("b2", (Cc,), 0.1)}
    m = n("x", (B, H * W, Cc))
    u = torch.nn.functional.linear(m, sd["m.fc1.weight"], sd["m.fc1.bias"]).reshape(B, H, W, 2 * half)
    g = ref_sgfn_gate(u, sd["m.dw.weight"], sd["m.dw.bias"], half)
    assert torch.equal(g[..., half:], u[..., half:])
    got = torch.nn.functional.linear(g.reshape(B, H * W, 2 * half), sd["m.fc2.weight"], sd["m.fc2.bias"])
    assert max_abs(got, O.sgfn(m, (H, W), sd, "m")) <= TOL


# ------------------------------------------------------------------------------------------------
# argument contract (include/hat_mi355x.h): HAT_EINVAL before anything is launched
# ------------------------------------------------------------------------------------------------
EINVAL = -1   # include/hat_mi355x.h
P = [C.c_void_p(0x1000 * (i + 1)) for i in range(5)]     # distinct non-null addresses: never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    import os
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load(), _lib


def _keybias(lib, *, sal=P[0], ldsal=8, ws=16, wse=24, pad=4, k_keep=345, dtype=None):
    return lib.hat_ocab_keybias(sal, ldsal, P[1], 288, P[2], 1, 48, 64, 144, ws, wse, pad, k_keep, dtype, None)


def test_keybias_refuses_bad_arguments(lib):
    lib, L = lib
    for dt in (L.HAT_F32, L.HAT_BF16):
        assert _keybias(lib, k_keep=0, dtype=dt) == EINVAL
        assert _keybias(lib, k_keep=-3, dtype=dt) == EINVAL
        assert _keybias(lib, wse=33, pad=9, dtype=dt) == EINVAL            # 33 * 33 > 1024 keys: one thread per key
        assert _keybias(lib, ldsal=0, dtype=dt) == EINVAL                  # a saliency map needs a row stride
    assert _keybias(lib, ldsal=-8, dtype=L.HAT_F32) == EINVAL              # the fp32 side map goes with bf16 kv only


def test_attention_kb_refuses_a_pad_that_is_not_the_ceiling(lib):
    lib, L = lib
    call = lambda ws, wse, pad, dt: lib.hat_ocab_attention_kb(P[0], P[1], P[2], P[3], P[4], 1, 48, 64, 144, 6, ws, wse, pad, 144, 288, 144, dt, None)
    for dt in (L.HAT_F32, L.HAT_BF16):
        for ws, wse, good in ((16, 24, 4), (16, 25, 5), (8, 12, 2), (8, 13, 3)):
            for pad in (good - 1, good + 1, 0, -1):
                assert call(ws, wse, pad, dt) == EINVAL


def test_attention_refuses_a_key_window_that_neither_fits_nor_streams(lib):
    """fp32, 24 x 24 queries and keys, d = 32: K + V^T take 82 944 + 74 240 B and the 47 x 47 table 8 836 B, 166 020 B in all
    against 163 840 B of LDS, and only 16 x 16 query windows stream: HAT_ELDS.  A 17 x 17 key window has no instantiation."""
    lib, L = lib
    ELDS, EUNSUPPORTED = -2, -3   # include/hat_mi355x.h
    plain = lambda ws, wse, dt: lib.hat_ocab_attention(P[0], P[1], P[2], P[4], 1, 48, 48, 64, 2, ws, wse, 64, 128, 64, dt, None)
    kb = lambda ws, wse, dt: lib.hat_ocab_attention_kb(P[0], P[1], P[2], P[3], P[4], 1, 48, 48, 64, 2, ws, wse, (wse - ws + 1) // 2,
                                                       64, 128, 64, dt, None)
    for call in (plain, kb):
        assert call(24, 24, L.HAT_F32) == ELDS
        for dt in (L.HAT_F32, L.HAT_BF16):
            assert call(16, 17, dt) == EUNSUPPORTED


def test_sgfn_gate_refuses_bad_arguments(lib):
    lib, L = lib
    call = lambda u, out, half, ldu, ldo, dt: lib.hat_sgfn_gate(u, P[1], P[2], out, 1, 8, 8, half, ldu, ldo, dt, None)
    for dt in (L.HAT_F32, L.HAT_BF16):
        assert call(P[0], P[0], 36, 72, 72, dt) == EINVAL                  # in place: the 3x3 taps would read written rows
        assert call(P[0], P[3], 38, 76, 76, dt) == EINVAL                  # four channels per thread
        assert call(P[0], P[3], 36, 71, 72, dt) == EINVAL                  # ldu < 2 * half (and not a multiple of 4)
        assert call(P[0], P[3], 36, 68, 72, dt) == EINVAL                  # ldu < 2 * half


def test_add_f32_refuses_a_length_that_is_not_a_multiple_of_four(lib):
    lib, L = lib
    for n in (1, 2, 3, 5, 1027):
        assert lib.hat_add_f32(P[0], P[1], P[2], 1, n, n, None) == EINVAL
        assert lib.hat_add_f32(P[0], P[1], P[2], 1, n, 0, None) == EINVAL
