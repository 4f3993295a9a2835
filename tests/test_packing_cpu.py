"""Host-side weight packing (super_resolution_amd/packing.py, reached as ops.pack_*), all on CPU tensors: every packer against the
bytes its predecessor produced (tests/golden/packing_digests.json), every layout against the formula include/hat_mi355x.h prints
for its buffer, applied directly to the unpacked weight, and the one fragment helper against a plain loop."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import GOLDEN
from super_resolution_amd import ops, packing

_spec = importlib.util.spec_from_file_location("gen_golden_packing", os.path.join(GOLDEN, "gen_golden_packing.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
Wt = gen.Wt
BF16, F32 = ops.HAT_BF16, ops.HAT_F32


def bf(t):
    return t.to(torch.bfloat16).float()


def asum(t):
    return float(t.double().abs().sum())


def acc_k(g, j):
    return 4 * g + j if j < 4 else 16 + 4 * g + j - 4


def check_elements(packed, want, idxs, what):
    assert len(idxs) >= 6
    for idx in idxs:
        assert float(packed[idx]) == float(want(*idx)), (what, idx, float(packed[idx]), float(want(*idx)))


def test_packers_match_parent_digests():
    """Every packer reproduces, bit for bit, what the packers produced before they shared one fragment helper: the fixture was
    written by gen_golden_packing.py from a checkout of that commit (its header says which)."""
    with open(os.path.join(GOLDEN, "packing_digests.json")) as f:
        fixture = json.load(f)
    assert "8c1ef91" in fixture["header"] and "dirty" not in fixture["header"]
    got = {name: gen.describe(p) for name, p in gen.pack_all(ops)}
    assert sorted(got) == sorted(fixture["cases"]) and len(got) == 22
    for name, want in fixture["cases"].items():
        assert got[name] == want, name


def test_packing_module_never_loads_the_library():
    """packing.py is host-only: importing it and packing a layer with the library path pointing nowhere works and loads nothing."""
    code = ("import torch; from super_resolution_amd import packing, _lib; "
            "p = packing.pack_pointwise(torch.ones(144, 144), None, _lib.HAT_BF16, 'cpu'); assert p.frag and _lib._lib is None")
    env = dict(os.environ, HAT_MI355X_LIB="/nonexistent/libhat_mi355x.so",
               PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] + sys.path))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_frag_helper_orders():
    """packing.frags on a 32 x 64 matrix holding 1000 row + col: natural order, accumulator order, and the 16-deep half step."""
    M = (1000 * torch.arange(32)[:, None] + torch.arange(64)[None, :]).float()
    nat, acc, half = packing.frags(M), packing.frags(M, "acc"), packing.frags(M[:, 48:], jn=4)
    assert nat.shape == acc.shape == (2, 2, 64, 8) and half.shape == (2, 1, 64, 4)
    for t in range(2):
        for lane in range(64):
            r, g = 16 * t + (lane & 15), lane >> 4
            for j in range(8):
                for ks in range(2):
                    assert float(nat[t, ks, lane, j]) == 1000 * r + 32 * ks + 8 * g + j
                    assert float(acc[t, ks, lane, j]) == 1000 * r + 32 * ks + acc_k(g, j)
                if j < 4:
                    assert float(half[t, 0, lane, j]) == 1000 * r + 48 + 4 * g + j


def test_pack_linear_weight_layout():
    """hat_linear (include/hat_mi355x.h): [n_slices][nt][ceil(Cin/32)][64][8], element (lane l, j) =
    W[slice*nt*16 + t*16 + (l & 15)][32*ks + 8*(l >> 4) + j], zero beyond Cin / n; two slices, ragged in both directions."""
    o, i = 300, 70
    W, b = Wt(o, i), Wt(o, k=3)
    pw = ops.pack_linear_weight(W, b, BF16, "cpu")
    assert (pw.nt, pw.n_slices, pw.kpad, pw.cin, pw.ksize, pw.nout, pw.frag) == (12, 2, 96, 70, 1, 300, True)
    assert pw.w.shape == (2, 12, 3, 64, 8) and pw.w.dtype == torch.bfloat16

    def want(s, t, ks, l, j):
        r, c = s * 192 + t * 16 + (l & 15), 32 * ks + 8 * (l >> 4) + j
        return bf(W)[r, c] if r < o and c < i else 0.0
    check_elements(pw.w, want, [(0, 0, 0, 0, 0), (1, 11, 2, 63, 7), (1, 3, 1, 37, 5), (0, 2, 2, 17, 0), (1, 6, 2, 11, 5), (1, 6, 2, 12, 5),
                                (0, 11, 0, 63, 7), (1, 0, 0, 0, 0)], "linear")
    assert asum(pw.w) == asum(bf(W))
    assert torch.equal(pw.bias[:o], b) and pw.bias.shape == (384,) and not pw.bias[o:].any()
    # a 3x3 weight is flattened tap-major first: K = tap * Cin_p + ci (hat_conv3x3_small)
    W3 = Wt(144, 6, 3, 3)
    p3 = ops.pack_linear_weight(W3, None, BF16, "cpu")
    assert (p3.nt, p3.n_slices, p3.kpad, p3.cin, p3.ksize) == (9, 1, 96, 6, 3)
    for (t, ks, l, j) in [(0, 0, 0, 0), (8, 2, 31, 5), (4, 1, 20, 3), (2, 0, 16, 6), (8, 2, 63, 7), (1, 2, 17, 0)]:
        r, k = 16 * t + (l & 15), 32 * ks + 8 * (l >> 4) + j
        tap, ci = k // 8, k % 8
        assert float(p3.w[0, t, ks, l, j]) == (float(bf(W3)[r, ci, tap // 3, tap % 3]) if tap < 9 and ci < 6 else 0.0)
    assert asum(p3.w) == asum(bf(W3)) and not p3.bias.any()


def test_pack_conv_weight_layout():
    """hat_conv: [Npad][Kpad] rows with K = tap * Cin_p + ci (Cin_p = Cin rounded up to 8), zero rows / columns past them;
    out_perm permutes the output channels (PixelShuffle), scale multiplies weight and bias."""
    W, b = Wt(20, 6, 3, 3), Wt(20, k=3)
    pw = ops.pack_conv_weight(W, b, BF16, "cpu")
    assert (pw.nt, pw.n_slices, pw.kpad, pw.cin, pw.ksize, pw.nout, pw.frag) == (4, 1, 128, 6, 3, 20, False)
    assert pw.w.shape == (64, 128) and pw.w.dtype == torch.bfloat16

    def want(n, k):
        tap, ci = k // 8, k % 8
        return bf(W)[n, ci, tap // 3, tap % 3] if n < 20 and tap < 9 and ci < 6 else 0.0
    check_elements(pw.w, want, [(0, 0), (19, 69), (5, 26), (19, 7), (20, 0), (63, 127), (3, 72), (7, 40)], "conv")
    assert asum(pw.w) == asum(bf(W))
    assert torch.equal(pw.bias[:20], b) and pw.bias.shape == (64,) and not pw.bias[20:].any()
    perm = gen.pixel_shuffle_perm(20, 2)
    pp = ops.pack_conv_weight(W, b, F32, "cpu", out_perm=perm, scale=0.5)
    for n in (0, 1, 7, 19):
        assert float(pp.w[n, 26]) == 0.5 * float(W[perm[n], 2, 1, 0]) and float(pp.bias[n]) == 0.5 * float(b[perm[n]])
    assert asum(pp.w) == 0.5 * asum(W)


def test_pack_ocab_mlp_layout():
    """HatMlpDesc: w1f = [18][4][64][8] (rows = hidden unit 16 nt + (lane & 15), k = 32 ks + 8 (lane >> 4) + j) followed by the
    16-deep tail [18][64][4] (k = 128 + 4 (lane >> 4) + j); w2f = [9][9][64][8], k-slot (g, j) of k-step kk = hidden unit
    32 kk + 4 g + j (j < 4) or 32 kk + 16 + 4 g + j - 4."""
    W1, b1, W2, b2 = Wt(288, 144), Wt(288, k=3), Wt(144, 288, k=5), Wt(144, k=7)
    p = ops.pack_ocab_mlp(W1, b1, W2, b2, "cpu")
    assert p.w1f.shape == (18 * 4 * 64 * 8 + 18 * 64 * 4,) and p.w2f.shape == (9, 9, 64, 8) and p.w1f.dtype == p.w2f.dtype == torch.bfloat16
    full, tail = p.w1f[:18 * 2048].reshape(18, 4, 64, 8), p.w1f[18 * 2048:].reshape(18, 64, 4)
    check_elements(full, lambda t, ks, l, j: bf(W1)[16 * t + (l & 15), 32 * ks + 8 * (l >> 4) + j],
                   [(0, 0, 0, 0), (17, 3, 63, 7), (5, 2, 37, 3), (17, 0, 15, 0), (0, 3, 48, 7), (9, 1, 16, 4)], "mlp fc1")
    check_elements(tail, lambda t, l, j: bf(W1)[16 * t + (l & 15), 128 + 4 * (l >> 4) + j],
                   [(0, 0, 0), (17, 63, 3), (5, 37, 2), (17, 15, 0), (0, 48, 3), (9, 16, 1)], "mlp fc1 tail")
    check_elements(p.w2f, lambda t, kk, l, j: bf(W2)[16 * t + (l & 15), 32 * kk + acc_k(l >> 4, j)],
                   [(0, 0, 0, 0), (8, 8, 63, 7), (3, 4, 37, 3), (3, 4, 37, 4), (8, 0, 15, 7), (0, 8, 48, 0)], "mlp fc2")
    assert asum(p.w1f) == asum(bf(W1)) and asum(p.w2f) == asum(bf(W2))
    assert torch.equal(p.b1, b1) and torch.equal(p.b2, b2) and (p.C, p.hidden) == (144, 288)


def test_pack_ocab_qkv_layout():
    """hat_ocab_qkv: the stacked weight [q_proj * qscale ; kv_proj] (432 x 144) in hat_ocab_mlp's fc1 layout ([27][4][64][8] +
    [27][64][4]); b1 [432] with the q part scaled likewise; a missing bias is zeros."""
    Wq, bq, Wkv = Wt(144, 144), Wt(144, k=3), Wt(288, 144, k=5)
    p = ops.pack_ocab_qkv(Wq, bq, Wkv, None, 0.2, "cpu")
    S = bf(torch.cat([Wq * 0.2, Wkv]))
    full, tail = p.w1f[:27 * 2048].reshape(27, 4, 64, 8), p.w1f[27 * 2048:].reshape(27, 64, 4)
    assert p.w1f.shape == (27 * 2048 + 27 * 256,) and p.w2f is None and p.b2 is None and (p.C, p.hidden) == (144, 432)
    check_elements(full, lambda t, ks, l, j: S[16 * t + (l & 15), 32 * ks + 8 * (l >> 4) + j],
                   [(0, 0, 0, 0), (26, 3, 63, 7), (8, 3, 15, 7), (9, 0, 0, 0), (14, 2, 37, 3), (26, 0, 16, 1)], "qkv")
    check_elements(tail, lambda t, l, j: S[16 * t + (l & 15), 128 + 4 * (l >> 4) + j],
                   [(0, 0, 0), (26, 63, 3), (8, 15, 3), (9, 0, 0), (14, 37, 2), (26, 16, 1)], "qkv tail")
    assert asum(p.w1f) == asum(S)
    assert torch.equal(p.b1[:144], bq * 0.2) and p.b1.shape == (432,) and not p.b1[144:].any()


def test_pack_cab_squeeze_layout():
    """hat_cab_squeeze: wpk [tile = 2 kx + j][kstep][64][8], fragment element [lane][e] = row lane % 16, input channel
    32 kstep + 8 (lane / 16) + e; j = 0: rows 0-7 = w[ch][.][ky=0][kx], rows 8-15 = w[ch][.][ky=1][kx]; j = 1: rows 0-7 =
    w[ch][.][ky=2][kx], rest 0; channels >= C and rows >= mid are zero.  bias: 8 floats, zeros past mid."""
    for mid, C_ in ((6, 144), (3, 64)):
        W, b = Wt(mid, C_, 3, 3), Wt(mid, k=3)
        wpk, b8 = ops.pack_cab_squeeze(W, b, "cpu")
        ks = -(-C_ // 32)
        assert wpk.shape == (6, ks, 64, 8) and wpk.dtype == torch.bfloat16

        def want(tile, kstep, l, e):
            row, ci, kx = l % 16, 32 * kstep + 8 * (l // 16) + e, tile // 2
            ky = (0 if row < 8 else 1) if tile % 2 == 0 else (2 if row < 8 else None)
            return bf(W)[row % 8, ci, ky, kx] if ky is not None and row % 8 < mid and ci < C_ else 0.0
        check_elements(wpk, want, [(0, 0, 0, 0), (5, ks - 1, 63, 7), (2, 1, 37, 3), (4, 0, 8, 0), (1, 1, 8 + 2, 5), (3, ks - 1, 48 + mid - 1, 7),
                                   (0, 0, mid, 0), (0, 0, 8 + mid - 1, 1), (5, 0, 2, 4), (4, ks - 1, 16 + mid - 1, (C_ - 1) % 8)], "squeeze")
        assert asum(wpk) == asum(bf(W))
        assert torch.equal(b8[:mid], b) and b8.shape == (8,) and not b8[mid:].any()


def test_pack_cab_w2f_is_the_expand_weight_in_fragment_order():
    """ops.pack_cab_w2f (HatCabFoldDesc.w2f, include/hat_mi355x.h): element (t, ks, lane, j) of the fp32 image is
    W2[16 t + lane % 16][ci = j][tap = 4 ks + lane // 16] (hat_arch.py:86's 3x3 expand conv) and zero where the output
    channel, the tap or the input channel does not exist — the order of hat_cab_fold's output, so that the kernel reads it
    with unit stride.  Host-side packing only: runs without a GPU."""
    g = torch.Generator().manual_seed(7)
    for C_, mid in ((144, 6), (160, 8), (136, 3)):
        w2 = torch.randn(C_, mid, 3, 3, generator=g)
        f = ops.pack_cab_w2f(w2, "cpu")
        nt = -(-C_ // 16)
        assert f.shape == (nt, 3, 64, 8) and f.dtype == torch.float32
        for (t, ks, lane, j) in [(0, 0, 0, 0), (nt - 1, 2, 63, 7), (3, 1, 17, 2), (nt - 1, 0, 15, mid - 1), (1, 2, 16, 0), (2, 2, 5, 1)]:
            co, tap = 16 * t + lane % 16, 4 * ks + lane // 16
            want = float(w2[co, j, tap // 3, tap % 3]) if (co < C_ and tap < 9 and j < mid) else 0.0
            assert float(f[t, ks, lane, j]) == want, (C_, mid, t, ks, lane, j)
        assert float(f.abs().sum()) == pytest.approx(float(w2.abs().sum()), rel=1e-6)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_pack_ffn_layout(dtype):
    """hat_ffn (HatFfnDesc), C = 24, hidden 48 padded to hid_p = 64 (two chunks):
    w1f [chunk][4][KS][64][8]: fc1 rows {a: 32c..32c+31, g: hid_p+32c..} of chunk c, K = round_up(C+1, 32), the fc1 bias as column C;
    w2f [chunk][nt][64][8]: fc2 columns 32c..32c+31, k order (g, j<4) -> 4g+j, (g, j>=4) -> 16+4g+j-4;
    dww [chunk][64][4 groups x 5 tap pairs]: the depthwise weight of channel (lane & 15) of each 16-channel group {a0, a1, g0, g1} for
    tap 2*pair + (lane >> 5), "tap 9" the depthwise bias, zero in lanes with ((lane & 15) >> 3) != ((lane >> 4) & 1); a bf16 is
    duplicated in both halves of a dword.  Every (unit, tap) lands in exactly one lane, so the non-zero lanes are the non-zero weights."""
    C_, hid = 24, 48
    W1, b1, Wd, bd, W2, b2 = gen.ffn_weights(C_, hid)
    p = ops.pack_ffn(W1, b1, Wd, bd, W2, b2, dtype, "cpu")
    r = bf if dtype == BF16 else (lambda t: t)
    assert (p.chunks, p.C, p.hid, p.nt, p.ks, p.layout) == (2, 24, 48, 2, 1, "ffn")
    assert p.w1f.shape == (2, 4, 1, 64, 8) and p.w2f.shape == (2, 2, 64, 8) and p.dww.shape == (2, 64, 20)

    def want1(c, t, ks, l, j):
        nl, col = 16 * t + (l & 15), 32 * ks + 8 * (l >> 4) + j
        unit = 32 * c + (nl & 31)
        row = (nl >> 5) * hid + unit
        return 0.0 if unit >= hid else r(W1)[row, col] if col < C_ else r(b1)[row] if col == C_ else 0.0
    check_elements(p.w1f, want1, [(0, 0, 0, 0, 0), (1, 3, 0, 63, 7), (0, 2, 0, 37, 3), (1, 0, 0, 48 + 15, 0), (1, 1, 0, 0, 0), (1, 2, 0, 48 + 15, 0),
                                  (0, 3, 0, 48 + 5, 0), (0, 1, 0, 48 + 5, 1), (1, 0, 0, 32 + 15, 7)], "ffn fc1")
    assert asum(p.w1f) == asum(r(W1)) + asum(r(b1))

    def want2(c, t, l, j):
        n, unit = 16 * t + (l & 15), 32 * c + acc_k(l >> 4, j)
        return r(W2)[n, unit] if n < C_ and unit < hid else 0.0
    check_elements(p.w2f, want2, [(0, 0, 0, 0), (1, 1, 63, 7), (0, 1, 7, 3), (0, 1, 8, 3), (1, 0, 48 + 3, 3), (1, 0, 48 + 3, 4), (1, 0, 0, 4),
                                  (0, 0, 37, 5)], "ffn fc2")
    assert asum(p.w2f) == asum(r(W2))
    Wd10 = r(torch.cat([Wd.reshape(-1, 9), bd[:, None]], 1))
    dww = p.dww if dtype == F32 else (p.dww & 0xFFFF).to(torch.int16).view(torch.bfloat16).float()
    if dtype == BF16:
        assert torch.equal(p.dww & 0xFFFF, (p.dww >> 16) & 0xFFFF) and p.dww.dtype == torch.int32

    def wantd(c, l, e):
        grp, pair = e // 5, e % 5
        unit, tap = 32 * c + 16 * (grp & 1) + (l & 15), 2 * pair + (l >> 5)
        return Wd10[(grp >> 1) * hid + unit, tap] if unit < hid and ((l & 15) >> 3) == ((l >> 4) & 1) else 0.0
    check_elements(dww, wantd, [(0, 0, 0), (1, 63, 19), (0, 37, 7), (0, 8, 0), (0, 24, 0), (1, 0, 5), (1, 0, 0), (1, 56, 14), (0, 40, 4),
                                (0, 63, 19)], "ffn dw")
    assert int((dww != 0).sum()) == int((Wd10 != 0).sum())
    for got, src in ((p.b1, b1), (p.dwb, bd)):
        assert torch.equal(got[:hid], src[:hid]) and torch.equal(got[64:64 + hid], src[hid:]) and not got[hid:64].any() and not got[64 + hid:].any()
    assert torch.equal(p.b2[:C_], b2) and p.b2.shape == (32,) and not p.b2[C_:].any()


def unit_of(c, t, l):
    """hat_ffn2 / hat_hab_tail3: fc1 output row (tile t, n16 = l & 15) of chunk c -> (half, hidden unit of that half)."""
    n = l & 15
    return t >> 1, 32 * c + 8 * (n >> 2) + 4 * (t & 1) + (n & 3)


def check_dw_record(rec, Wd10, hid, chunks, what):
    """[chunk][4 groups][10][16]: hidden units 32c+8g..+7 per tap 0..8 and the depthwise bias as "tap 9": eight a-unit values then
    eight gate-unit values (zero units past hid)."""
    def want(c, g, tap, e):
        unit = 32 * c + 8 * g + (e & 7)
        return Wd10[(e >> 3) * hid + unit, tap] if unit < hid else 0.0
    check_elements(rec, want, [(0, 0, 0, 0), (chunks - 1, 3, 9, 15), (1, 2, 4, 5), (1, 2, 4, 13), (0, 3, 9, 0), (chunks - 1, 3, 0, 7),
                               (chunks - 1, 0, 8, 8), (chunks - 1, 1, 9, 7)], what)
    assert asum(rec) == asum(Wd10)


def test_pack_ffn2_layout():
    """hat_ffn2 (include/hat_mi355x.h), C = 144, hidden 64 (two chunks):
    w1f [chunk][4][5][64][8] bf16: fc1 rows {a | gate: hid+..} of chunk c in the kernel's unit order, K = 144 zero padded to 160, NO
    bias column;  b1 [chunk][64] fp32: the fc1 bias of the chunk's rows in the same order;  dww [chunk][4][10][16] fp16;
    w2f [chunk][9][64][8] fp16: fc2 columns 32c..32c+31 in natural k order (k = 8*(lane>>4) + j);  b2 [144] fp32."""
    C_, hid = 144, 64
    W1, b1, Wd, bd, W2, b2 = gen.ffn_weights(C_, hid)
    p = ops.pack_ffn2(W1, b1, Wd, bd, W2, b2, "cpu")
    assert (p.chunks, p.C, p.hid, p.nt, p.ks, p.layout) == (2, 144, 64, 9, 5, "ffn2")
    assert p.w1f.shape == (2, 4, 5, 64, 8) and p.w1f.dtype == torch.bfloat16 and p.w2f.shape == (2, 9, 64, 8) and p.w2f.dtype == torch.float16
    assert p.dww.shape == (2, 4, 10, 16) and p.dww.dtype == torch.float16 and p.b1.shape == (2, 64)

    def want1(c, t, ks, l, j):
        half, unit = unit_of(c, t, l)
        col = 32 * ks + 8 * (l >> 4) + j
        return bf(W1)[half * hid + unit, col] if col < C_ else 0.0
    check_elements(p.w1f, want1, [(0, 0, 0, 0, 0), (1, 3, 4, 63, 7), (0, 1, 2, 37, 3), (1, 2, 4, 16 + 9, 7), (1, 2, 4, 32 + 9, 0), (0, 1, 0, 4, 0),
                                  (0, 0, 0, 4, 0), (1, 3, 4, 15, 7)], "ffn2 fc1")
    assert asum(p.w1f) == asum(bf(W1))
    for (c, t, l) in [(0, 0, 0), (1, 3, 15), (0, 1, 6), (1, 2, 9), (0, 2, 0), (1, 0, 4)]:
        half, unit = unit_of(c, t, l)
        assert float(p.b1[c, 16 * t + l]) == float(b1[half * hid + unit])
    assert asum(p.b1) == asum(b1)
    check_elements(p.w2f, lambda c, t, l, j: W2.half()[16 * t + (l & 15), 32 * c + 8 * (l >> 4) + j],
                   [(0, 0, 0, 0), (1, 8, 63, 7), (0, 4, 37, 3), (1, 0, 15, 0), (0, 8, 48, 7), (1, 3, 16, 4)], "ffn2 fc2")
    assert asum(p.w2f) == asum(W2.half())
    check_dw_record(p.dww, torch.cat([Wd.reshape(-1, 9), bd[:, None]], 1).half(), hid, 2, "ffn2 dw")
    assert torch.equal(p.b2, b2) and torch.equal(p.dwb, bd)


def test_pack_ffn3_layout():
    """hat_hab_tail3 at embed_dim 180 (include/hat_mi355x.h): w1f [12][4][6][64][8] as for hat_ffn2 but with LayerNorm2's gamma
    folded into the columns and the fc1 bias W1 @ beta + b1 as column k = 180; hidden 360 zero padded to 384; w2f [12][12][64][8]
    (channel tile 11 holds 180..191: rows past 180 zero); dww [12][1024]: hat_ffn2's 640-element record zero padded; b2 [256]."""
    C_, hid, hid_p = 180, 360, 384
    W1, b1, Wd, bd, W2, b2 = gen.ffn_weights(C_, hid)
    gam, bet = Wt(C_, k=17), Wt(C_, k=19)
    p = ops.pack_ffn3(W1, b1, Wd, bd, W2, b2, gam, bet, "cpu")
    assert (p.chunks, p.C, p.hid, p.nt, p.ks, p.layout) == (12, 180, 360, 12, 6, "tail3")
    assert p.w1f.shape == (12, 4, 6, 64, 8) and p.w1f.dtype == torch.bfloat16 and p.w2f.shape == (12, 12, 64, 8) and p.w2f.dtype == torch.float16
    assert p.dww.shape == (12, 1024) and p.dww.dtype == torch.float16 and p.b2.shape == (256,)
    Wg = bf(W1 * gam[None, :])                                     # one fp32 rounding per element, then the bf16 one: exact to restate
    bias64 = W1.double() @ bet.double() + b1.double()              # the bias column: compared to bf16 precision (2^-8 relative)

    def want1(c, t, ks, l, j):
        half, unit = unit_of(c, t, l)
        col = 32 * ks + 8 * (l >> 4) + j
        return Wg[half * hid + unit, col] if unit < hid and col < C_ else 0.0
    check_elements(p.w1f, want1, [(0, 0, 0, 0, 0), (11, 3, 5, 63, 7), (5, 1, 2, 37, 3), (11, 0, 0, 4, 0), (11, 0, 0, 3, 0), (3, 2, 5, 32 + 7, 5),
                                  (3, 2, 5, 32 + 7, 3), (11, 1, 5, 15, 3), (7, 3, 0, 0, 0)], "tail3 fc1")
    for (c, t, l) in [(0, 0, 0), (11, 2, 3), (5, 1, 6), (10, 3, 15), (3, 2, 9), (11, 1, 7)]:       # column 180 = k-step 5, g = 2, j = 4
        half, unit = unit_of(c, t, l)
        got, want = float(p.w1f[c, t, 5, 32 + (l & 15), 4]), (float(bias64[half * hid + unit]) if unit < hid else 0.0)
        assert abs(got - want) <= 2.0 ** -8 * abs(want) + 1e-30, (c, t, l, got, want)
    assert asum(p.w1f) == pytest.approx(asum(Wg) + asum(bf(bias64.float())), rel=1e-6)
    assert not p.w1f.reshape(12, 4, 6, 4, 16, 8)[:, :, 5, 2, :, 5:].any() and not p.w1f[:, :, 5, 48:].any()    # columns 181..191

    def want2(c, t, l, j):
        n, unit = 16 * t + (l & 15), 32 * c + 8 * (l >> 4) + j
        return W2.half()[n, unit] if n < C_ and unit < hid else 0.0
    check_elements(p.w2f, want2, [(0, 0, 0, 0), (11, 11, 63, 7), (5, 4, 37, 3), (11, 0, 16, 7), (11, 0, 32, 0), (3, 11, 3, 0), (3, 11, 4, 0),
                                  (11, 11, 3, 7)], "tail3 fc2")
    assert asum(p.w2f) == asum(W2.half())
    check_dw_record(p.dww[:, :640].reshape(12, 4, 10, 16), torch.cat([Wd.reshape(-1, 9), bd[:, None]], 1).half(), hid, 12, "tail3 dw")
    assert not p.dww[:, 640:].any()
    assert torch.equal(p.b2[:C_], b2) and not p.b2[C_:].any()
    assert p.b1.shape == p.dwb.shape == (4,) and not p.b1.any() and not p.dwb.any()
    # embed_dim 144: the same record shapes with nine channel tiles and five k-steps, the bias in column 144
    W1, b1, Wd, bd, W2, b2 = gen.ffn_weights(144, 64)
    p = ops.pack_ffn3(W1, b1, Wd, bd, W2, b2, torch.ones(144), torch.zeros(144), "cpu")
    q2 = ops.pack_ffn2(W1, b1, Wd, bd, W2, b2, "cpu")
    assert torch.equal(p.w2f, q2.w2f) and torch.equal(p.dww[:, :640].reshape(2, 4, 10, 16), q2.dww)
    w1 = p.w1f.clone()
    assert torch.equal(w1[:, :, 4, 32:48, 0].float().reshape(2, 64), bf(q2.b1))     # column 144 = k-step 4, g = 2, j = 0
    w1[:, :, 4, 32:48, 0] = 0
    assert torch.equal(w1, q2.w1f)


def test_pack_pointwise_chooses_the_instantiated_kernel():
    """hat_linear's packing where ops.linear_supported, hat_conv's otherwise; the flag comes from the constructors."""
    for (o, i) in ((144, 144), (288, 144), (180, 720), (100, 36)):
        W, b = Wt(o, i), Wt(o, k=3)
        p = ops.pack_pointwise(W, b, BF16, "cpu", scale=0.5)
        ref = (ops.pack_linear_weight if ops.linear_supported(o, i, BF16) else ops.pack_conv_weight)(W, b, BF16, "cpu", scale=0.5)
        assert p.frag == ops.linear_supported(o, i, BF16) == ref.frag
        assert torch.equal(p.w, ref.w) and torch.equal(p.bias, ref.bias) and (p.nt, p.n_slices, p.kpad) == (ref.nt, ref.n_slices, ref.kpad)
    assert ops.pack_pointwise(Wt(144, 144), None, BF16, "cpu").frag and not ops.pack_pointwise(Wt(180, 720), None, BF16, "cpu").frag
