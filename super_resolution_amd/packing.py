"""Host-side weight packing: state-dict tensors -> the layouts the kernels read (include/hat_mi355x.h).  Pure index
gathering on CPU tensors; nothing here loads the library or touches the GPU (`device` is only where the result is put).

Every MFMA A-fragment layout goes through `frags`; a packer builds the padded matrix (bias column, zero hidden units),
reorders its rows where the layout has a row permutation, calls `frags`, and reshapes to the documented dimension order.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import HAT_BF16, HAT_F32

TORCH_DTYPE = {HAT_F32: torch.float32, HAT_BF16: torch.bfloat16}
KC = {HAT_F32: 32, HAT_BF16: 64}


class PackedConv:
    """Packed weights of one conv/linear layer (see HatConvDesc in include/hat_mi355x.h)."""
    __slots__ = ("w", "bias", "ksize", "cin", "kpad", "nt", "n_slices", "nout", "w_bstride", "frag", "ksplit")

    def __init__(self, w, bias, ksize, cin, kpad, nt, n_slices, nout, w_bstride=0, frag=False):
        self.w, self.bias, self.ksize, self.cin, self.kpad = w, bias, ksize, cin, kpad
        self.nt, self.n_slices, self.nout, self.w_bstride = nt, n_slices, nout, w_bstride
        self.frag = frag  # True: MFMA-fragment order for hat_linear; False: [Npad][Kpad] rows for hat_conv
        self.ksplit = None  # second half of a layer whose K is split over two launches (engine._lin)

    @property
    def npad(self):
        return self.nt * 16 * self.n_slices


class PackedMlp:
    """fc1 / fc2 of the OCAB's MLP in hat_ocab_mlp's fragment layouts (include/hat_mi355x.h)."""
    __slots__ = ("w1f", "b1", "w2f", "b2", "C", "hidden")


class PackedFFN:
    """GatedDconvFFN weights; `layout` names the kernel generation they are packed for: "ffn" (hat_ffn), "ffn2" (hat_ffn2 /
    hat_hab_tail) or "tail3" (hat_hab_tail3)."""
    __slots__ = ("w1f", "b1", "dww", "dwb", "w2f", "b2", "chunks", "C", "hid", "nt", "ks", "layout")


def choose_nt(nout: int):
    """n-tiles per slice in {12, 9, 8, 4, 1}: least padded work, weighted by LDS fragment reads per MFMA."""
    best = None
    for nt in (12, 9, 8, 4, 1):
        npad = -(-nout // (16 * nt)) * 16 * nt
        cost = npad * (nt + 2) / nt
        if best is None or cost < best[0]:
            best = (cost, nt, npad // (16 * nt))
    return best[1], best[2]


def choose_nt_linear(nout: int, cin: int, dtype: int):
    """hat_linear's n-tiling: like choose_nt, except that a 288-wide output over 144 inputs (OCAB kv and MLP fc1 of the
    embed_dim-144 models) is ONE slice of 18 n-tiles in bf16 (90 KB of weights in LDS): every slice re-reads the input,
    and these layers are HBM-bound."""
    if nout == 288 and -(-cin // 32) == 5 and dtype == HAT_BF16:
        return 18, 1
    if nout == 360 and -(-cin // 32) == 6 and dtype == HAT_BF16:   # the same layers of the embed_dim-180 models: 23 n-tiles, 138 KB
        return 23, 1
    return choose_nt(nout)


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).cpu()


def _pad(m: torch.Tensor, rows: int, cols: Optional[int] = None) -> torch.Tensor:
    """m (a vector or a matrix) zero padded to `rows` rows (and `cols` columns)."""
    if m.dim() == 1:
        out = torch.zeros(rows)
        out[:m.shape[0]] = m
    else:
        out = torch.zeros(rows, m.shape[1] if cols is None else cols)
        out[:m.shape[0], :m.shape[1]] = m
    return out


def frags(M: torch.Tensor, order: str = "natural", jn: int = 8) -> torch.Tensor:
    """MFMA A fragments of a 2-D fp32 matrix (rows a multiple of 16, columns a multiple of 4 jn): [rows/16][cols/(4 jn)][64][jn]
    with element (t, ks, lane, j) = M[16 t + (lane & 15)][4 jn ks + k(lane >> 4, j)], k(g, j) = jn g + j ("natural": the 32-deep
    k-step with jn = 8, the 16-deep half step with jn = 4) or j < 4 ? 4 g + j : 16 + 4 g + j - 4 ("acc": the accumulator order
    of the stage that produced the operand, jn = 8).  A view: callers convert and make it contiguous."""
    assert M.dim() == 2 and M.shape[0] % 16 == 0 and M.shape[1] % (4 * jn) == 0 and (order == "natural" or (order, jn) == ("acc", 8))
    lane, j = torch.arange(64)[:, None], torch.arange(jn)[None, :]
    g = lane >> 4
    k = jn * g + j if order == "natural" else torch.where(j < 4, 4 * g + j, 16 + 4 * g + j - 4)
    return M.reshape(M.shape[0] // 16, 16, M.shape[1] // (4 * jn), 4 * jn)[:, lane & 15, :, k].permute(2, 3, 0, 1)


def _tap_major(w: torch.Tensor) -> torch.Tensor:
    """(O, I, k, k) -> (O, k*k*Cin_p) with K = tap * Cin_p + ci, Cin_p = I rounded up to 8 (zero channels)."""
    o, i, kh, kw = w.shape
    assert kh == kw
    wt = torch.zeros(o, kh * kw, (i + 7) // 8 * 8)
    wt[:, :, :i] = w.permute(0, 2, 3, 1).reshape(o, kh * kw, i)
    return wt.reshape(o, -1)


# ------------------------------------------------------------------------------------------------
# hat_conv / hat_linear / hat_conv3x3_small
# ------------------------------------------------------------------------------------------------
def pack_conv_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], dtype: int, device, out_perm=None,
                     scale: float = 1.0, nt: Optional[int] = None) -> PackedConv:
    """weight (O, I, k, k) [or (O, I) for nn.Linear] -> [Npad][Kpad] with K = tap * Cin_p + ci."""
    w = _f32(weight)
    if w.dim() == 2:
        w = w[:, :, None, None]
    o, i, kh, _ = w.shape
    b = torch.zeros(o) if bias is None else _f32(bias)
    if scale != 1.0:
        w, b = w * scale, b * scale
    if out_perm is not None:
        w, b = w[out_perm], b[out_perm]
    w = _tap_major(w)
    if nt is None:
        nt, n_slices = choose_nt(o)
    else:
        n_slices = -(-o // (16 * nt))
    kc = KC[dtype] * (3 if nt == 1 else (2 if nt <= 4 else 1))  # weight chunk length of hat_conv.hip: longer for few n-tiles
    kpad = -(-w.shape[1] // kc) * kc
    npad = nt * 16 * n_slices
    return PackedConv(_pad(w, npad, kpad).to(TORCH_DTYPE[dtype]).to(device).contiguous(), _pad(b, npad).to(device), kh, i, kpad, nt, n_slices, o)


def pack_linear_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], dtype: int, device, scale: float = 1.0) -> PackedConv:
    """weight (O, I) -> MFMA A-fragment order [n_slices][nt][ceil(I/32)][64 lanes][8] for hat_linear (include/hat_mi355x.h:
    element (lane l, j) = W[slice*nt*16 + t*16 + (l & 15)][32*ks + 8*(l >> 4) + j], zero beyond Cin / n).
    A conv weight (O, I, k, k) is first flattened to K = tap * Cin_p + ci (hat_conv3x3_small)."""
    w = _f32(weight)
    ksize, cin = 1, None
    if w.dim() == 4 and w.shape[-1] > 1:
        cin, ksize = w.shape[1], w.shape[2]
        w = _tap_major(w)
    w = w.reshape(w.shape[0], -1) * scale
    o, i = w.shape
    b = (torch.zeros(o) if bias is None else _f32(bias)) * scale
    nt, n_slices = choose_nt_linear(o, i, dtype) if ksize == 1 else choose_nt(o)
    ks = -(-i // 32)
    npad = nt * 16 * n_slices
    wf = frags(_pad(w, npad, ks * 32)).reshape(n_slices, nt, ks, 64, 8)
    return PackedConv(wf.to(TORCH_DTYPE[dtype]).contiguous().to(device), _pad(b, npad).to(device), ksize, (i if cin is None else cin),
                      ks * 32, nt, n_slices, o, frag=True)


def pack_pointwise(weight: torch.Tensor, bias: Optional[torch.Tensor], dtype: int, device, scale: float = 1.0) -> PackedConv:
    """A pointwise layer for hat_linear when its shape is instantiated (PackedConv.frag), else for hat_conv (ksize 1)."""
    from .ops import linear_supported   # which kernels exist is the launch wrappers' knowledge
    if linear_supported(weight.shape[0], weight.shape[1], dtype):
        return pack_linear_weight(weight, bias, dtype, device, scale=scale)
    return pack_conv_weight(weight, bias, dtype, device, scale=scale)


# ------------------------------------------------------------------------------------------------
# hat_ocab_mlp / hat_ocab_qkv
# ------------------------------------------------------------------------------------------------
def _pack_fc1_frags(W1: torch.Tensor) -> torch.Tensor:
    """(16 nt, 144) fp32 -> hat_ocab_mlp's fc1 layout: [nt][4][64 lanes][8] full k-steps (k = 32 ks + 8 g + j) then
    [nt][64][4] the 16-deep tail (k = 128 + 4 g + j)."""
    return torch.cat([frags(W1[:, :128]).reshape(-1), frags(W1[:, 128:], jn=4).reshape(-1)])


def pack_ocab_mlp(fc1_w, fc1_b, fc2_w, fc2_b, device) -> PackedMlp:
    """HatMlpDesc (include/hat_mi355x.h): w1f = fc1 as A fragments [18][4][64][8] + the 16-deep tail [18][64][4];
    w2f = fc2 as A fragments [9 n-tiles][9 k-steps][64][8], k-slot (g, j) of k-step kk = hidden unit 32 kk + 4 g + j (j < 4) or
    32 kk + 16 + 4 g + j - 4 (the accumulator order of fc1's results)."""
    W1, b1, W2, b2 = _f32(fc1_w), _f32(fc1_b), _f32(fc2_w), _f32(fc2_b)
    hid, C_ = W1.shape
    assert (C_, hid) == (144, 288) and W2.shape == (C_, hid)
    p = PackedMlp()
    p.w1f = _pack_fc1_frags(W1).to(torch.bfloat16).contiguous().to(device)
    p.w2f = frags(W2, "acc").to(torch.bfloat16).contiguous().to(device)
    p.b1, p.b2, p.C, p.hidden = b1.contiguous().to(device), b2.contiguous().to(device), C_, hid
    return p


def pack_ocab_qkv(q_w, q_b, kv_w, kv_b, qscale: float, device) -> PackedMlp:
    """Stacked [q_proj * qscale ; kv_proj] (432 x 144) for hat_ocab_qkv, in hat_ocab_mlp's fc1 layout ([27][4][64][8] + [27][64][4])."""
    Wq, Wkv = _f32(q_w) * qscale, _f32(kv_w)
    bq = (torch.zeros(Wq.shape[0]) if q_b is None else _f32(q_b)) * qscale
    bkv = torch.zeros(Wkv.shape[0]) if kv_b is None else _f32(kv_b)
    W = torch.cat([Wq, Wkv], 0)
    assert W.shape == (432, 144)
    p = PackedMlp()
    p.w1f = _pack_fc1_frags(W).to(torch.bfloat16).contiguous().to(device)
    p.b1 = torch.cat([bq, bkv]).contiguous().to(device)
    p.w2f = p.b2 = None
    p.C, p.hidden = 144, 432
    return p


# ------------------------------------------------------------------------------------------------
# CAB: the row-sweep squeeze conv (hat_cab_squeeze / hat_conv3x3_to_*) and hat_cab_fold's w2f
# ------------------------------------------------------------------------------------------------
def pack_cab_squeeze(weight: torch.Tensor, bias: torch.Tensor, device):
    """3x3 weight (mid <= 8, C, 3, 3) -> the 6 x ceil(C/32) MFMA A fragments the row-sweep kernel keeps in registers
    (hat_cab_squeeze / hat_conv3x3_to_planes: wpk [tile = 2 kx + j][kstep][64 lanes][8] bf16, j = 0: rows 0-7 = ky 0,
    rows 8-15 = ky 1; j = 1: rows 0-7 = ky 2, rest zero), + 8 bias floats."""
    w = _f32(weight)
    mid, cin = w.shape[0], w.shape[1]
    A = torch.zeros(6, 16, 32 * -(-cin // 32))       # [tile][row][k]
    for kx in range(3):
        A[2 * kx, 0:mid, :cin] = w[:, :, 0, kx]      # ky = 0 -> output row r + 1
        A[2 * kx, 8:8 + mid, :cin] = w[:, :, 1, kx]  # ky = 1 -> output row r
        A[2 * kx + 1, 0:mid, :cin] = w[:, :, 2, kx]  # ky = 2 -> output row r - 1
    return frags(A.reshape(96, -1)).to(torch.bfloat16).contiguous().to(device), _pad(_f32(bias), 8).to(device)


def pack_cab_w2f(w2: torch.Tensor, device) -> torch.Tensor:
    """(C, mid <= 8, 3, 3) expand-conv weight -> fp32 [nt][3][64][8] in the order of hat_cab_fold's output `wf` (HatCabFoldDesc.w2f):
    element (t, ks, lane, j) = W2[16 t + (lane & 15)][ci = j][tap = 4 ks + (lane >> 4)], the fragments of the [co][tap * 8 + ci] matrix."""
    w = _f32(w2)
    C_, mid = w.shape[0], w.shape[1]
    full = torch.zeros(-(-C_ // 16) * 16, 12, 8)           # [co][tap 0..11][ci 0..7]
    full[:C_, :9, :mid] = w.reshape(C_, mid, 9).permute(0, 2, 1)
    return frags(full.reshape(-1, 96)).contiguous().to(device)


# ------------------------------------------------------------------------------------------------
# the gated depthwise FFN: hat_ffn, hat_ffn2 / hat_hab_tail, hat_hab_tail3
# ------------------------------------------------------------------------------------------------
FP16_SAFE = 6.0e4   # below _Float16's largest finite value, 65504


def ffn_fp16_range_bound(fc1_w, fc1_b, dw_w, dw_b, ln_g, ln_b) -> float:
    """Worst-case magnitude of anything hat_ffn2 / hat_hab_tail3 hold in FP16 — the hidden tensor u = fc1(LayerNorm2(x)), the
    depthwise conv's outputs a and g, and the gated product a * g * sigmoid(g) — for ANY input: LayerNorm's normalised row
    has Euclidean norm <= sqrt(C), so |u_j| <= sqrt(C) * ||W1[j] * gamma||_2 + |W1[j] . beta + b1[j]| =: U_j (Cauchy-Schwarz),
    |a_j| <= sum_taps |wd[j, tap]| * U_j + |bd_j|, likewise g, and |a * g * sigmoid(g)| <= |a| * |g|.
    The kernels convert to FP16 with round-toward-zero (a value past the range saturates at 65504 instead of becoming an
    infinity) but the packed-FP16 products behind that conversion can still overflow, so the engine uses these kernels only
    while this bound stays below FP16_SAFE and otherwise keeps hat_ffn (hidden tensor in bf16, fp32 range).  The bound is loose
    by design (a trained HAT-S sits orders of magnitude below it: unit-variance rows, weights of norm ~1 give U ~ 12, a * g ~ 10^3)."""
    f = lambda t: t.detach().to(torch.float64).cpu()
    W1, b1, Wd, bd, g_, b_ = f(fc1_w), f(fc1_b), f(dw_w).reshape(-1, 9), f(dw_b), f(ln_g), f(ln_b)
    C_ = W1.shape[1]
    hid = W1.shape[0] // 2
    U = (C_ ** 0.5) * (W1 * g_[None, :]).norm(dim=1) + (W1 @ b_ + b1).abs()
    A = Wd.abs().sum(1) * U + bd.abs()
    return float(max(U.max(), A.max(), (A[:hid] * A[hid:]).max()))


def _halves(m: torch.Tensor, hid_p: int) -> torch.Tensor:
    """[a half ; gate half] (2 hid rows) with each half zero padded to hid_p rows (zero hidden units)."""
    hid = m.shape[0] // 2
    return torch.cat([_pad(m[:hid], hid_p), _pad(m[hid:], hid_p)])


def _ffn_rows(chunks: int, unit_order: bool) -> torch.Tensor:
    """Row of the [a ; gate] matrix (hid_p = 32 chunks rows per half) that fc1 output row nl = 16 tile + n16 of chunk c computes
    (tiles 0, 1: a half; 2, 3: gate half): (chunks, 64).  Plain order: unit 32 c + (nl & 31) of its half (hat_ffn).  Unit order:
    unit 32 c + 8 (n16 >> 2) + 4 (tile & 1) + (n16 & 3), so that a lane's 4 + 4 results of the two tiles are 16 contiguous bytes of
    the U row, unit order natural (one ds_write_b128, hat_ffn2.hip `ust`)."""
    nl = torch.arange(64)
    q = 8 * ((nl & 15) >> 2) + 4 * ((nl >> 4) & 1) + (nl & 3) if unit_order else nl & 31
    return (nl >> 5)[None, :] * (32 * chunks) + torch.arange(chunks)[:, None] * 32 + q[None, :]


def _ffn_fc1(W1, b1, chunks: int, ks: int, unit_order: bool) -> torch.Tensor:
    """w1f [chunk][4][ks][64 lanes][8]: the fragments of the chunk's 64 fc1 rows (_ffn_rows), K zero padded to 32 ks, with the
    fc1 bias as column k = C where b1 is given (the kernel keeps a constant 1 in k-slot C of the normalised activations)."""
    M = _pad(_halves(W1, 32 * chunks), 64 * chunks, 32 * ks)
    if b1 is not None:
        M[:, W1.shape[1]] = _halves(b1, 32 * chunks)
    return frags(M[_ffn_rows(chunks, unit_order).reshape(-1)]).reshape(chunks, 4, ks, 64, 8)


def _ffn_fc2(W2, nt: int, chunks: int, order: str) -> torch.Tensor:
    """w2f [chunk][nt][64 lanes][8]: fc2 columns 32 c .. 32 c + 31 of output-channel tile nt, in `order` (frags)."""
    return frags(_pad(W2, 16 * nt, 32 * chunks), order).permute(1, 0, 2, 3)


def _ffn_dw_record(Wd, bd, chunks: int) -> torch.Tensor:
    """[chunk][g][tap 0..8, the depthwise bias as "tap 9"][a-units 32 c + 8 g .. + 7 | gate-units 32 c + 8 g .. + 7] (hat_ffn2's dww)."""
    Wd10 = _halves(torch.cat([Wd, bd[:, None]], dim=1), 32 * chunks)        # (2 hid_p, 10)
    return Wd10.reshape(2, chunks, 4, 8, 10).permute(1, 2, 4, 0, 3).reshape(chunks, 4, 10, 16)


def _ffn_args(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b):
    W1, b1, Wd, bd, W2, b2 = _f32(fc1_w), _f32(fc1_b), _f32(dw_w).reshape(-1, 9), _f32(dw_b), _f32(fc2_w), _f32(fc2_b)
    C_, hid = W2.shape
    assert W1.shape == (2 * hid, C_) and Wd.shape[0] == 2 * hid
    return W1, b1, Wd, bd, W2, b2, C_, hid, -(-hid // 32)


def _packed_ffn(layout, w1f, w2f, dww, b1, dwb, b2, chunks, C_, hid, nt, ks, device) -> PackedFFN:
    p = PackedFFN()
    p.w1f, p.w2f, p.dww = w1f.contiguous().to(device), w2f.contiguous().to(device), dww.contiguous().to(device)
    p.b1, p.dwb, p.b2 = b1.contiguous().to(device), dwb.to(device), b2.to(device)
    p.chunks, p.C, p.hid, p.nt, p.ks, p.layout = chunks, C_, hid, nt, ks, layout
    return p


def pack_ffn(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b, dtype: int, device) -> PackedFFN:
    """Fragment-pack GatedDconvFFN weights (hat_arch.py:99-104) for hat_ffn; layouts in include/hat_mi355x.h (HatFfnDesc):
      w1f [chunk][4][ks][64][8]: fc1 rows {a: 32c..32c+31, g: hid_p+32c..} of chunk c, K = round_up(C + 1, 32) with the fc1
          bias as column k = C;
      w2f [chunk][nt][64][8]: fc2 columns 32c..32c+31, k in the accumulator order of the depthwise stage: element (g, j<4) <->
          channel 4g+j of a-group 0, (g, j>=4) <-> channel 16+4g+(j-4);
      dww [chunk][64 lanes][4 groups x 5 tap pairs]: one value per (chunk, lane, group of 16 channels {a0, a1, g0, g1}, tap pair):
          lane (n = l & 15, g = l >> 4) owns channel n of the group and tap 2*pair + (g >> 1) (tap 9 = the depthwise BIAS,
          multiplied by a constant 1 in the kernel); non-zero only in the lanes whose 8-wide k group holds channel n
          (n >> 3 == g & 1), so the kernel builds its diagonal A fragment from this single value.  bf16: stored duplicated in
          both halves of a dword;
      b1, dwb [2 hid_p], b2 [16 nt]: zero padded fp32."""
    W1, b1, Wd, bd, W2, b2, C_, hid, chunks = _ffn_args(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b)
    hid_p = 32 * chunks
    ks = -(-(C_ + 1) // 32)          # K padded to a multiple of 32 with room for the bias column at k = C
    nt = 9 if C_ == 144 else (12 if C_ == 180 else 2)
    tdt = TORCH_DTYPE[dtype]
    lane = torch.arange(64)
    n16, g4 = lane & 15, lane >> 4
    Wd10 = _halves(torch.cat([Wd, bd[:, None]], dim=1), hid_p).reshape(2, chunks, 2, 16, 10)   # [a | gate][chunk][16-group][ch][tap]
    tap = 2 * torch.arange(5)[None, :] + (g4[:, None] >> 1)                  # (64, 5)
    active = ((n16 >> 3) == (g4 & 1)).to(torch.float32)                      # (64,)
    dww = Wd10[:, :, :, n16[:, None], tap] * active[:, None]                 # (2, chunks, 2, 64, 5)
    dww = dww.permute(1, 3, 0, 2, 4).reshape(chunks, 64, 20)
    if dtype == HAT_BF16:
        bits = dww.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
        dww = (bits | (bits << 16)).to(torch.int32)
    return _packed_ffn("ffn", _ffn_fc1(W1, b1, chunks, ks, False).to(tdt), _ffn_fc2(W2, nt, chunks, "acc").to(tdt), dww,
                       _halves(b1, hid_p), _halves(bd, hid_p), _pad(b2, nt * 16), chunks, C_, hid, nt, ks, device)


def pack_ffn2(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b, device) -> PackedFFN:
    """GatedDconvFFN weights (hat_arch.py:99-104) in hat_ffn2's layouts (include/hat_mi355x.h):
      w1f [chunk][4][5][64][8] bf16: fc1 rows of chunk c in unit order (_ffn_rows), K = 144 zero padded to 160, NO bias column;
      b1 [chunk][64] fp32: the fc1 bias of the chunk's rows in the same order;
      dww [chunk][4][10][16] fp16 (_ffn_dw_record);  w2f [chunk][9][64][8] fp16, natural k order;  b2 [144] fp32."""
    W1, b1, Wd, bd, W2, b2, C_, hid, chunks = _ffn_args(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b)
    assert hid % 32 == 0 and C_ == 144
    ks, nt = 5, 9
    return _packed_ffn("ffn2", _ffn_fc1(W1, None, chunks, ks, True).to(torch.bfloat16), _ffn_fc2(W2, nt, chunks, "natural").to(torch.float16),
                       _ffn_dw_record(Wd, bd, chunks).to(torch.float16), b1[_ffn_rows(chunks, True)], bd, _pad(b2, nt * 16),
                       chunks, C_, hid, nt, ks, device)


def pack_ffn3(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b, ln_g, ln_b, device) -> PackedFFN:
    """GatedDconvFFN weights (hat_arch.py:99-104) + the affine part of the LayerNorm in front of them (norm2, hat_arch.py:237)
    in hat_hab_tail3's layouts (include/hat_mi355x.h), embed_dim 144 or 180:
      * LayerNorm2's gamma folded into the fc1 columns and W1 . beta into the fc1 bias (fc1(xhat * gamma + beta) =
        (W1 diag(gamma)) xhat + (W1 beta + b1), exact in real arithmetic): the kernel normalises without an affine step;
      * the fc1 bias as column k = C of the fc1 fragments (K = C + 1 padded to a multiple of 32);
      * the hidden width padded to a multiple of 32 with zero units (embed_dim 180: 360 -> 384);
      * fc1 output row (tile, n16) of a chunk computes hidden unit 8 (n16 >> 2) + 4 (tile & 1) + (n16 & 3) of its half, so that a
        lane's 4 + 4 results of the two tiles are 16 contiguous bytes of the U row (as pack_ffn2);
      * the depthwise record of a chunk zero padded to 2 KiB and the fc2 bias to 1 KiB (every record the kernel copies is then
        a whole number of 1 KiB LDS-DMA pieces)."""
    W1, b1, Wd, bd, W2, b2, C_, hid, chunks = _ffn_args(fc1_w, fc1_b, dw_w, dw_b, fc2_w, fc2_b)
    gam, bet = _f32(ln_g), _f32(ln_b)
    assert C_ in (144, 180)
    b1 = b1 + W1 @ bet
    W1 = W1 * gam[None, :]
    ks, nt = (C_ + 1 + 31) // 32, (C_ + 15) // 16
    dww = _pad(_ffn_dw_record(Wd, bd, chunks).reshape(chunks, 640), chunks, 1024)
    return _packed_ffn("tail3", _ffn_fc1(W1, b1, chunks, ks, True).to(torch.bfloat16), _ffn_fc2(W2, nt, chunks, "natural").to(torch.float16),
                       dww.to(torch.float16), torch.zeros(4), torch.zeros(4), _pad(b2, 256), chunks, C_, hid, nt, ks, device)


# ------------------------------------------------------------------------------------------------
# the NAF stem of HybridHATNAF: hat_naf_half / hat_naf_fold (hybrid_hat_naf_arch.py:16-82)
# ------------------------------------------------------------------------------------------------
NAF_WIDTHS = (64, 32)   # channel counts hat_naf_half is instantiated for


class PackedNafBlock:
    """One NAFBlock in hat_naf_half's / hat_naf_fold's operand layouts (include/hat_mi355x.h "NAF stem"): per half the (2c, c)
    1x1 as A fragments [2c/16][c/32][64][8] T (w1), its bias [2c], the depthwise taps [9][2c] and bias [2c], all fp32; the
    attention half's fold inputs wsca, w2 [c][c], bsca, b2, beta [c] fp32 (hat_naf_fold makes Wf per sample); the FFN half's
    static fold wf2 = T fragments of gamma * ffn2.weight [c/16][c/32][64][8], bf2 = gamma * ffn2.bias [c] fp32."""
    __slots__ = ("w1", "b1", "dww", "dwb", "wsca", "bsca", "w2", "b2", "beta", "w1f", "b1f", "dwwf", "dwbf", "wf2", "bf2")


def naf_frags(M: torch.Tensor, dtype: int, device) -> torch.Tensor:
    """A (rows, c) matrix of a NAF 1x1 conv -> hat_naf_half's A fragments [rows/16][c/32][64][8] of type T."""
    return frags(M).to(TORCH_DTYPE[dtype]).contiguous().to(device)


def naf_ffn_fold(gamma: torch.Tensor, ffn2_w: torch.Tensor, ffn2_b: torch.Tensor):
    """out = y + gamma * ffn2(g2) as y + Wf . g2 + bf: Wf = gamma[o] * W[o][i], bf = gamma * b (fp32, host)."""
    gam = _f32(gamma).reshape(-1)
    W = _f32(ffn2_w).reshape(gam.shape[0], -1)
    return gam[:, None] * W, gam * _f32(ffn2_b)


def pack_naf_block(sd, p: str, dtype: int, device) -> PackedNafBlock:
    """sd[p + '.pw1.weight'] ... of one NAFBlock (state-dict names of hybrid_hat_naf_arch.py:27-46) -> PackedNafBlock."""
    c = sd[p + ".beta"].numel()
    if c not in NAF_WIDTHS:
        raise ValueError(f"naf_width {c} is not supported: hat_naf_half is built for {' and '.join(map(str, NAF_WIDTHS))} channels")
    vec = lambda k: _f32(sd[p + k]).reshape(-1).contiguous().to(device)
    mat = lambda k: _f32(sd[p + k]).reshape(sd[p + k].shape[0], -1)
    taps = lambda k: _f32(sd[p + k]).reshape(2 * c, 9).t().contiguous().to(device)
    b = PackedNafBlock()
    b.w1, b.b1, b.dww, b.dwb = naf_frags(mat(".pw1.weight"), dtype, device), vec(".pw1.bias"), taps(".dw.weight"), vec(".dw.bias")
    b.wsca, b.bsca = mat(".sca.1.weight").contiguous().to(device), vec(".sca.1.bias")
    b.w2, b.b2, b.beta = mat(".pw2.weight").contiguous().to(device), vec(".pw2.bias"), vec(".beta")
    b.w1f, b.b1f, b.dwwf, b.dwbf = naf_frags(mat(".ffn1.weight"), dtype, device), vec(".ffn1.bias"), taps(".ffn_dw.weight"), vec(".ffn_dw.bias")
    wf2, bf2 = naf_ffn_fold(sd[p + ".gamma"], sd[p + ".ffn2.weight"], sd[p + ".ffn2.bias"])
    b.wf2, b.bf2 = naf_frags(wf2, dtype, device), bf2.contiguous().to(device)
    return b


# ------------------------------------------------------------------------------------------------
# ESC: hat_esc_convffn (esc_arch.py:148-159) and the geometric re-parameterisation of the large-kernel filter (:289-298)
# ------------------------------------------------------------------------------------------------
ESC_HID_PAD = {80: 96, 128: 128}   # hidden widths hat_esc_convffn is instantiated for -> padded to a multiple of 32


class PackedEscFfn:
    """One ConvFFN in hat_esc_convffn's operand layouts (include/hat_mi355x.h "ESC"): w1 T fragments [hid_p/16][2][64][8] of the
    (hid_p, 64) 1x1, w2 T fragments [4][hid_p/32][64][8] of the (64, hid_p) 1x1, b1 / dwb [hid_p], dww [9][hid_p], b2 [64] fp32; the
    pad units are zero everywhere."""
    __slots__ = ("w1", "b1", "dww", "dwb", "w2", "b2", "hid", "hid_p")


def pack_esc_convffn(sd, p: str, dtype: int, device) -> PackedEscFfn:
    """sd[p + '.proj.weight'] ... of one ConvFFN (state-dict names of esc_arch.py:151-153) -> PackedEscFfn."""
    W1 = _f32(sd[p + ".proj.weight"])
    hid, dim = W1.shape[0], W1.shape[1]
    if dim != 64 or hid not in ESC_HID_PAD:
        raise ValueError(f"ConvFFN {dim} -> {hid} is not supported: hat_esc_convffn is built for 64 channels and a hidden width of "
                         f"{' or '.join(map(str, ESC_HID_PAD))} (exp_ratio 1.25 or 2)")
    hp = ESC_HID_PAD[hid]
    f = PackedEscFfn()
    f.hid, f.hid_p = hid, hp
    f.w1 = frags(_pad(W1.reshape(hid, dim), hp)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b1 = _pad(_f32(sd[p + ".proj.bias"]), hp).to(device)
    f.dww = _pad(_f32(sd[p + ".dwc.weight"]).reshape(hid, 9), hp).t().contiguous().to(device)
    f.dwb = _pad(_f32(sd[p + ".dwc.bias"]), hp).to(device)
    f.w2 = frags(_pad(_f32(sd[p + ".aggr.weight"]).reshape(dim, hid), dim, hp)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b2 = _f32(sd[p + ".aggr.bias"]).contiguous().to(device)
    return f


class _ESC:
    """Packed parameters of one ConvAttnWrapper (esc_arch.py:136-145) + its large-kernel filter."""

    def __init__(self, sd, core: str, plk_key: str, pdim: int, ksize: int, C: int, dtype: int, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.pdim, self.ksize = pdim, ksize
        self.w1 = sd[core + ".plk.dwc_proj.1.weight"].detach().reshape(pdim // 2, pdim).to(**f32).contiguous()
        self.b1 = sd[core + ".plk.dwc_proj.1.bias"].detach().to(**f32).contiguous()
        self.w2 = sd[core + ".plk.dwc_proj.3.weight"].detach().reshape(pdim * 9, pdim // 2).to(**f32).contiguous()
        self.b2 = sd[core + ".plk.dwc_proj.3.bias"].detach().to(**f32).contiguous()
        # static large-kernel filter packed in fp32 [16 or 32][Kpad]; hat_esc_weights adds the dynamic
        # depthwise 3x3 on the diagonal of the central taps and casts to T per forward
        lk = pack_conv_weight(sd[plk_key], None, HAT_F32, dev, nt=1)
        kc = KC[dtype] * 3  # nt == 1 chunk length (hat_conv.hip)
        self.kpad = -(-(ksize * ksize * ((pdim + 7) // 8 * 8)) // kc) * kc
        self.npad = 16 if pdim <= 16 else 32   # weight rows / output channels of the conv (one or two 16-row slices)
        plk = torch.zeros(self.npad, self.kpad, **f32)
        plk[:lk.w.shape[0], :min(self.kpad, lk.kpad)] = lk.w[:self.npad, :min(self.kpad, lk.kpad)]
        self.plk = plk.contiguous()
        self.zero_bias = torch.zeros(self.npad, **f32)
        self.aggr = None  # packed by the engine (hat_linear when the shape is instantiated)
        self.aggr_keys = (core + ".aggr.weight", core + ".aggr.bias")
        self.conv13 = False   # set by the engine: the conv runs on hat_esc_conv13 (else on hat_conv)


ESCFP_HID_PAD = {60: 64, 72: 96, 96: 96}   # hidden widths hat_escfp_convffn is instantiated for (48 channels) -> padded


def pack_escfp_convffn(sd, p: str, dtype: int, device) -> PackedEscFfn:
    """One ConvFFN of ESCFP (esc_fp_arch.py:139-150) in hat_escfp_convffn's operand layouts (include/hat_mi355x.h "ESCFP"): as
    pack_esc_convffn at 48 channels, with W1's 48 columns zero-padded to the two k-steps (64) the kernel runs: w1 [hid_p/16][2][64][8],
    w2 [3][hid_p/32][64][8], b2 [48]."""
    W1 = _f32(sd[p + ".proj.weight"])
    hid, dim = W1.shape[0], W1.shape[1]
    if dim != 48 or hid not in ESCFP_HID_PAD:
        raise ValueError(f"ConvFFN {dim} -> {hid} is not supported: hat_escfp_convffn is built for 48 channels and a hidden width of "
                         f"{', '.join(map(str, ESCFP_HID_PAD))} (exp_ratio 1.25, 1.5 or 2)")
    hp = ESCFP_HID_PAD[hid]
    f = PackedEscFfn()
    f.hid, f.hid_p = hid, hp
    f.w1 = frags(_pad(W1.reshape(hid, dim), hp, 64)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b1 = _pad(_f32(sd[p + ".proj.bias"]), hp).to(device)
    f.dww = _pad(_f32(sd[p + ".dwc.weight"]).reshape(hid, 9), hp).t().contiguous().to(device)
    f.dwb = _pad(_f32(sd[p + ".dwc.bias"]), hp).to(device)
    f.w2 = frags(_pad(_f32(sd[p + ".aggr.weight"]).reshape(dim, hid), dim, hp)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b2 = _f32(sd[p + ".aggr.bias"]).contiguous().to(device)
    return f


class PackedEscFpLk:
    """hat_escfp_weights' operands for one DecomposedConvolutionalAttention (esc_fp_arch.py:89-120), all fp32: w1 (4,16), b1 [4],
    w2 (144,4), b2 [144] = plk.proj.1 / plk.proj.3; lk_channel (16,16), lk_spatial (16,169) = the network's two shared filters.  kpad:
    the row length of the weight image it writes = what hat_esc_conv13 / hat_conv (nt 1) read for a 13 x 13 conv over 16 channels."""
    __slots__ = ("w1", "b1", "w2", "b2", "lk_channel", "lk_spatial", "kpad", "zero_bias", "aggr", "conv13")   # the last two: set by the engine


def pack_escfp_lk(sd, p: str, dtype: int, device) -> PackedEscFpLk:
    """sd[p + '.plk.proj.1.weight'] ..., sd['lk_channel'], sd['lk_spatial'] -> PackedEscFpLk."""
    w1, w2 = _f32(sd[p + ".plk.proj.1.weight"]), _f32(sd[p + ".plk.proj.3.weight"])
    lc, ls = _f32(sd["lk_channel"]), _f32(sd["lk_spatial"])
    if tuple(w1.shape[:2]) != (4, 16) or tuple(w2.shape[:2]) != (144, 4) or tuple(lc.shape) != (16, 16, 1, 1) or tuple(ls.shape) != (16, 1, 13, 13):
        raise ValueError(f"large-kernel branch {tuple(w1.shape)} / {tuple(w2.shape)} / {tuple(lc.shape)} / {tuple(ls.shape)} is not supported: "
                         "hat_escfp_weights is built for pdim 16 (16 -> 4 -> 144) and a 13 x 13 kernel")
    f = PackedEscFpLk()
    f.w1, f.b1 = w1.reshape(4, 16).contiguous().to(device), _f32(sd[p + ".plk.proj.1.bias"]).contiguous().to(device)
    f.w2, f.b2 = w2.reshape(144, 4).contiguous().to(device), _f32(sd[p + ".plk.proj.3.bias"]).contiguous().to(device)
    f.lk_channel, f.lk_spatial = lc.reshape(16, 16).contiguous().to(device), ls.reshape(16, 169).contiguous().to(device)
    kc = KC[dtype] * 3   # hat_conv's weight chunk length at nt == 1
    f.kpad = -(-(169 * 16) // kc) * kc
    f.zero_bias = torch.zeros(16, device=device)
    return f


def escfp_rank1_fold(lk_channel, k):
    """lk_channel (16,16,1,1), k (16,1,13,13) = lk_spatial + the padded dynamic kernel -> the dense (16,16,13,13) filter
    weff[o][i] = lk_channel[o][i] * k[o] of conv1x1(lk_channel) followed by the depthwise conv k.  lk_channel has no bias, so zero
    padding commutes with it and the dense conv with zero padding 6 is exact at the border too."""
    return lk_channel.reshape(16, 16, 1, 1) * k.reshape(16, 1, 13, 13)


def bicubic_phase_table(s: int) -> torch.Tensor:
    """(s, 4) fp32: the weights of F.interpolate(scale_factor=s, mode='bicubic', align_corners=False) per output phase p = o % s, on
    the source taps o // s + first .. first + 3 with first = -2 if 2 p + 1 < s else -1: Keys' cubic with A = -0.75 at the exact
    fraction t = frac((2 p + 1) / (2 s) - 1/2), computed in fp64."""
    A = -0.75
    inner = lambda t: ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0           # |t| <= 1
    outer = lambda t: ((A * t - 5.0 * A) * t + 8.0 * A) * t - 4.0 * A     # 1 < |t| < 2
    rows = []
    for p in range(s):
        num = (2 * p + 1 - s) % (2 * s)     # t = num / (2 s), exactly
        t = num / (2.0 * s)
        rows.append([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)])
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def esc_geo_ensemble(k: torch.Tensor) -> torch.Tensor:
    """The mean of the 8 flips / rotations of a (pdim, pdim, k, k) filter, in the reference's order of additions (esc_arch.py:289-298)."""
    r = torch.rot90(k, -1, [2, 3])
    return (k + k.flip([3]) + k.flip([2]) + k.flip([2, 3]) + r + r.flip([3]) + r.flip([2]) + r.flip([2, 3])) / 8


# ------------------------------------------------------------------------------------------------
# ESCReal (esc_real_arch.py:402-475): the three pack-time folds.  Each fold function computes in the dtype of its arguments
# (the packers pass fp32; the tests pass fp64 to pin the identities to round-off).
# ------------------------------------------------------------------------------------------------
def escreal_skip_fold(w0, b0, dw, bdw):
    """skip.0 (1x1 3 -> 128) followed by skip.1 (depthwise 7x7, reflect padding) as ONE dense 7x7 conv 3 -> 128 on the
    reflect-padded image: reflect padding leaves no tap outside, so Wf[c][ci][ky][kx] = dw[c][ky][kx] * W0[c][ci] and the bias is
    the constant b0[c] * sum_tap dw[c][tap] + bdw[c].  -> (Wf (128, 3, 7, 7), bf (128,))."""
    c = w0.shape[0]
    d = dw.reshape(c, 1, 7, 7)
    return d * w0.reshape(c, 3, 1, 1), b0 * d.sum((1, 2, 3)) + bdw


def nearest_conv_fold(w, b):
    """UpsamplingNearest2d(2) -> Conv2d(I, O, 3, 1, 1) as Conv2d(I, 4 O, 3, 1, 1) at the low size -> PixelShuffle(2): for output
    phase (i, j) every HR tap's weight is added onto the LR tap it lands on — rows {-1 | 0, +1} for i = 0, {-1, 0 | +1} for i = 1,
    columns alike — and the output channel is 4 c + 2 i + j.  Zero padding agrees at every border: an HR tap outside the x2 map
    lands on an LR tap outside the map.  -> (weight (4 O, I, 3, 3), bias (4 O,))."""
    o, i = w.shape[:2]
    m = torch.tensor([[[1, 0, 0], [0, 1, 1], [0, 0, 0]], [[0, 0, 0], [1, 1, 0], [0, 0, 1]]], dtype=w.dtype)   # [phase][LR tap][HR tap]
    wf = torch.einsum("iak,jbl,cnkl->cijnab", m, m, w).reshape(4 * o, i, 3, 3)
    return wf, b.repeat_interleave(4)


def dysample_fold(offset_w, offset_b, scope_w, end_w, groups: int = 4):
    """DySample's three pointwise layers as one: rows [offset 8 s^2 | scope 8 s^2 (no bias) | proj 3 groups], proj[3 g + o] =
    end_conv.weight[o] restricted to group g's channels — end_conv in front of the (linear) sampling; end_conv.bias joins after
    it (the four bilinear weights of a group sum to 1, and the bias counts once, not once per group).
    -> (weight (16 s^2 + 3 groups, C), bias)."""
    c = offset_w.shape[1]
    cg = c // groups
    ew = end_w.reshape(end_w.shape[0], c)
    proj = torch.zeros(groups * ew.shape[0], c, dtype=ew.dtype)
    for g in range(groups):
        proj[ew.shape[0] * g: ew.shape[0] * (g + 1), cg * g: cg * (g + 1)] = ew[:, cg * g: cg * (g + 1)]
    w = torch.cat([offset_w.reshape(-1, c), scope_w.reshape(-1, c), proj], 0)
    return w, torch.cat([offset_b, torch.zeros(w.shape[0] - offset_b.shape[0], dtype=offset_b.dtype)])


class PackedEscRealSkip:
    """The skip branch in hat_escreal_skip's operand layouts (include/hat_mi355x.h "ESCReal"): w1 T fragments [8][5][64][8] of the
    folded (128, 160) matrix (column 3 tap + ci, 147.. zero), b1 [128], w3 T fragments [4][4][64][8] of the (64, 128) 1x1, b3 [64]."""
    __slots__ = ("w1", "b1", "w3", "b3")


def pack_escreal_skip(sd, p: str, dtype: int, device) -> PackedEscRealSkip:
    """sd[p + '.0.weight'] ... of ESCReal.skip (esc_real_arch.py:460-465) -> PackedEscRealSkip."""
    w0, dw, w3 = _f32(sd[p + ".0.weight"]), _f32(sd[p + ".1.weight"]), _f32(sd[p + ".3.weight"])
    if tuple(w0.shape) != (128, 3, 1, 1) or tuple(dw.shape) != (128, 1, 7, 7) or tuple(w3.shape) != (64, 128, 1, 1):
        raise ValueError(f"skip branch {tuple(w0.shape)} / {tuple(dw.shape)} / {tuple(w3.shape)} is not supported: hat_escreal_skip is "
                         "built for 3 -> 128 (1x1), depthwise 7x7, 128 -> 64 (1x1)")
    wf, bf = escreal_skip_fold(w0, _f32(sd[p + ".0.bias"]), dw, _f32(sd[p + ".1.bias"]))
    f = PackedEscRealSkip()
    f.w1 = frags(_pad(wf.permute(0, 2, 3, 1).reshape(128, 147), 128, 160)).to(TORCH_DTYPE[dtype]).contiguous().to(device)   # k = 3 tap + ci
    f.b1 = bf.contiguous().to(device)
    f.w3 = frags(w3.reshape(64, 128)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b3 = _f32(sd[p + ".3.bias"]).contiguous().to(device)
    return f


def pack_nearest_conv(weight, bias, dtype: int, device) -> PackedConv:
    """nearest x2 + 3x3 conv -> the folded conv for hat_conv with HAT_O_PIXSHUF_T (ps_r = 2): output channel 4 c + ij is stored as
    packed row ij * O + c, HATEngine's Upsample layout."""
    wf, bf = nearest_conv_fold(_f32(weight), _f32(bias))
    o = weight.shape[0]
    n = torch.arange(4 * o)
    return pack_conv_weight(wf, bf, dtype, device, out_perm=(n % o) * 4 + n // o)


# ------------------------------------------------------------------------------------------------
# ESCRealM (esc_real_arch.py:478-661): the unshuffled stem's skip branch and the heads of UniUpsample
# ------------------------------------------------------------------------------------------------
UNI_UPSAMPLERS = ("conv", "pixelshuffledirect", "pixelshuffle", "nearest+conv", "dysample")   # SampleMods, in MetaUpsample's index order


class PackedEscRealMSkip:
    """The skip branch over 12 or 48 unshuffled channels in hat_escrealm_skip's layouts (include/hat_mi355x.h "ESCRealM"): w0 fp32
    [128][cin], b0 [128], dw fp32 [128][49], bdw [128], w3 T fragments [4][4][64][8] of the (64, 128) 1x1, b3 [64]."""
    __slots__ = ("cin", "w0", "b0", "dw", "bdw", "w3", "b3")


def pack_escrealm_skip(sd, p: str, dtype: int, device) -> PackedEscRealMSkip:
    """sd[p + '.1.weight'] ... of ESCRealM.skip behind its PixelUnshuffle (esc_real_arch.py:613-619) -> PackedEscRealMSkip."""
    w0, dw, w3 = _f32(sd[p + ".1.weight"]), _f32(sd[p + ".2.weight"]), _f32(sd[p + ".4.weight"])
    cin = w0.shape[1]
    if cin not in (12, 48) or tuple(w0.shape) != (128, cin, 1, 1) or tuple(dw.shape) != (128, 1, 7, 7) or tuple(w3.shape) != (64, 128, 1, 1):
        raise ValueError(f"skip branch {tuple(w0.shape)} / {tuple(dw.shape)} / {tuple(w3.shape)} is not supported: hat_escrealm_skip is "
                         "built for 12 or 48 -> 128 (1x1), depthwise 7x7, 128 -> 64 (1x1)")
    f = PackedEscRealMSkip()
    f.cin = cin
    f.w0, f.b0 = w0.reshape(128, cin).contiguous().to(device), _f32(sd[p + ".1.bias"]).contiguous().to(device)
    f.dw, f.bdw = dw.reshape(128, 49).contiguous().to(device), _f32(sd[p + ".2.bias"]).contiguous().to(device)
    f.w3 = frags(w3.reshape(64, 128)).to(TORCH_DTYPE[dtype]).contiguous().to(device)
    f.b3 = _f32(sd[p + ".4.bias"]).contiguous().to(device)
    return f


def pixshuf_perm(o: int, r: int) -> torch.Tensor:
    """Row order of a conv whose o = r^2 c outputs feed PixelShuffle(r) through HAT_O_PIXSHUF_T: packed row ij * c + cc holds
    nn.PixelShuffle's channel cc * r^2 + ij."""
    n = torch.arange(o)
    cps = o // (r * r)
    return (n % cps) * (r * r) + n // cps


def conv_nearest_fold(w, b, r: int):
    """Conv2d(I, O, 3, 1, 1) -> nn.Upsample(scale_factor=r) (nearest) as Conv2d(I, r^2 O, 3, 1, 1) -> PixelShuffle(r): every one of
    the r^2 output pixels of an LR pixel is that pixel's conv result, so output channel c r^2 + ij repeats row c.  Exact: no
    arithmetic changes, and a pointwise activation behind the nearest step acts on the same values in the conv's epilogue.
    (UniUpsample's "nearest+conv" puts the conv FIRST, esc_real_arch.py:514-544; ESCReal's own head upsamples first, which is
    nearest_conv_fold.)  -> (weight (r^2 O, I, 3, 3), bias (r^2 O,))."""
    return w.repeat_interleave(r * r, 0), b.repeat_interleave(r * r)


def pack_conv_nearest(weight, bias, r: int, dtype: int, device) -> PackedConv:
    """3x3 conv + nearest x r -> the folded conv for hat_conv with HAT_O_PIXSHUF_T (ps_r = r)."""
    if r not in (2, 3):
        raise ValueError(f"nearest x{r} is not supported: the fold is built for 2 and 3")
    wf, bf = conv_nearest_fold(_f32(weight), _f32(bias), r)
    return pack_conv_weight(wf, bf, dtype, device, out_perm=pixshuf_perm(wf.shape[0], r))


def pack_pixshuf_conv(weight, bias, r: int, dtype: int, device) -> PackedConv:
    """Conv2d(I, r^2 C, 3, 1, 1) in front of nn.PixelShuffle(r) for hat_conv with HAT_O_PIXSHUF_T (ps_r = r)."""
    return pack_conv_weight(weight, bias, dtype, device, out_perm=pixshuf_perm(weight.shape[0], r))


# ------------------------------------------------------------------------------------------------
# hat_lte_query (ESC-LTE's head)
# ------------------------------------------------------------------------------------------------
LTE_HIDDEN = 256   # hidden_dim and every entry of hidden_list hat_lte_query is built for


class PackedLte:
    """The LTE head for hat_lte_query: `taps` the coef | freq 3x3 convs as ONE hat_conv layer of 512 outputs (fp32 rows out),
    `phase` fp32 [128][2], `w` / `b` the three hidden layers (T fragments [16][8][64][8], fp32 [256]), `w4` / `b4` the last layer in fp32."""
    __slots__ = ("taps", "phase", "w", "b", "w4", "b4")


def pack_lte(sd, dtype: int, device) -> PackedLte:
    """sd: coef.*, freq.*, phase.weight, imnet.layers.{0,2,4,6}.* of the reference's LTE (esc_arb/models/lte.py:14-21)."""
    hd = LTE_HIDDEN
    if tuple(sd["coef.weight"].shape[:1]) != (hd,) or tuple(sd["freq.weight"].shape[:1]) != (hd,) or tuple(sd["phase.weight"].shape) != (hd // 2, 2):
        raise ValueError(f"ESC-LTE with hidden_dim={sd['coef.weight'].shape[0]} is not supported: hat_lte_query is built for hidden_dim {hd}")
    shapes = [tuple(sd[f"imnet.layers.{i}.weight"].shape) for i in (0, 2, 4, 6) if f"imnet.layers.{i}.weight" in sd]
    if shapes != [(hd, hd)] * 3 + [(3, hd)] or "imnet.layers.8.weight" in sd:
        raise ValueError(f"ESC-LTE with an imnet of layer shapes {shapes} is not supported: hat_lte_query is built for hidden_list "
                         f"({hd}, {hd}, {hd}) and out_dim 3")
    p = PackedLte()
    p.taps = pack_conv_weight(torch.cat([_f32(sd["coef.weight"]), _f32(sd["freq.weight"])]),
                              torch.cat([_f32(sd["coef.bias"]), _f32(sd["freq.bias"])]), dtype, device)
    p.phase = _f32(sd["phase.weight"]).contiguous().to(device)
    p.w = [frags(_f32(sd[f"imnet.layers.{i}.weight"])).to(TORCH_DTYPE[dtype]).contiguous().to(device) for i in (0, 2, 4)]
    p.b = [_f32(sd[f"imnet.layers.{i}.bias"]).contiguous().to(device) for i in (0, 2, 4)]
    p.w4 = _f32(sd["imnet.layers.6.weight"]).contiguous().to(device)
    p.b4 = _f32(sd["imnet.layers.6.bias"]).contiguous().to(device)
    return p


# ------------------------------------------------------------------------------------------------
# hat_upfold_* (the last PixelShuffle(2) conv and conv_last as one 5x5 conv at the shuffle's input size)
# ------------------------------------------------------------------------------------------------
class PackedUpfold:
    """`w` T fragments [12 variants][50][64][8], `bias` fp32 [12][16]; variant 3 rs + cs (upfold_variant), fragment 2 t + ks of tap
    t = 5 (ty + 2) + (tx + 2), A row 4 (2 a + b) + m (m < 3; row 4 (2 a + b) + 3 is zero): lane group g of the MFMA result holds
    R, G, B of output pixel 2 p + (g >> 1, g & 1)."""
    __slots__ = ("w", "bias")


def upfold_pieces(wu, bu, wl, bl):
    """Conv2d(C, 4 K, 3, 1, 1) -> PixelShuffle(2) -> Conv2d(K, M, 3, 1, 1) as per-shift pieces, in fp64.  Tap d of the last conv
    at output pixel 2 p + (a, b) reads shuffled pixel 2 (p + delta) + (a', b'), delta = floor((a + d) / 2), a' = (a + d) mod 2:
      y[m, 2 p + (a, b)] = bl[m] + sum_delta [p + delta inside] (B[delta][m, a, b] + sum_e sum_c G[delta][m, a, b, c, e] x[c, p + delta + e])
    -> G (3, 3, M, 2, 2, C, 3, 3) indexed [delta_y + 1, delta_x + 1, m, a, b, c, e_y + 1, e_x + 1], B (3, 3, M, 2, 2), bl (M,)."""
    wu, bu, wl, bl = (t.detach().to(torch.float64).cpu() for t in (wu, bu, wl, bl))
    m, k = wl.shape[:2]
    if wu.shape[0] != 4 * k or tuple(wu.shape[2:]) != (3, 3) or tuple(wl.shape[2:]) != (3, 3):
        raise ValueError(f"upfold: a {tuple(wu.shape)} conv does not feed PixelShuffle(2) and a {tuple(wl.shape)} conv")
    c = wu.shape[1]
    wu4, bu4 = wu.reshape(k, 4, c, 3, 3), bu.reshape(k, 4)
    G, Bd = torch.zeros(3, 3, m, 2, 2, c, 3, 3, dtype=torch.float64), torch.zeros(3, 3, m, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    iy, ix, sub = (a + dy) // 2 + 1, (b + dx) // 2 + 1, 2 * ((a + dy) % 2) + (b + dx) % 2
                    G[iy, ix, :, a, b] += torch.einsum("mk,kcef->mcef", wl[:, :, dy + 1, dx + 1], wu4[:, sub])
                    Bd[iy, ix, :, a, b] += wl[:, :, dy + 1, dx + 1] @ bu4[:, sub]
    return G, Bd, bl


def upfold_variant(G, Bd, bl, rs: int, cs: int):
    """The merged 5x5 weights F (M, 2, 2, C, 5, 5) = sum over the shifts delta present of G[delta] placed at delta + e, and the bias
    (M, 2, 2) = bl + their B[delta], for a pixel p whose neighbour rows / columns are partly outside the image: rs bit 0: row
    p_y - 1 is outside (the first row), bit 1: row p_y + 1 is (the last row); cs likewise for columns.  (0, 0) is the interior."""
    m, c = G.shape[2], G.shape[5]
    F = torch.zeros(m, 2, 2, c, 5, 5, dtype=torch.float64)
    bias = bl[:, None, None].expand(m, 2, 2).clone()
    for iy in range(3):
        for ix in range(3):
            if (iy == 0 and rs & 1) or (iy == 2 and rs & 2) or (ix == 0 and cs & 1) or (ix == 2 and cs & 2):
                continue
            F[..., iy:iy + 3, ix:ix + 3] += G[iy, ix]
            bias += Bd[iy, ix]
    return F, bias


def upfold_apply(x, wu, bu, wl, bl):
    """The fold applied on the host in fp64, every pixel by its variant: x (B, C, H, W) -> (B, M, 2 H, 2 W).  What hat_upfold_*
    computes, for the tests."""
    x = x.detach().to(torch.float64).cpu()
    G, Bd, b0 = upfold_pieces(wu, bu, wl, bl)
    Bn, _, H, W = x.shape
    m = G.shape[2]
    py, px = torch.arange(H)[:, None], torch.arange(W)[None, :]
    rs, cs = (py == 0) * 1 + (py == H - 1) * 2, (px == 0) * 1 + (px == W - 1) * 2
    out = torch.zeros(Bn, m * 4, H, W, dtype=torch.float64)
    for r in range(4):
        for s in range(4):
            mask = (rs == r) & (cs == s)
            if mask.any():
                F, bias = upfold_variant(G, Bd, b0, r, s)
                y = torch.nn.functional.conv2d(x, F.reshape(m * 4, -1, 5, 5), bias.reshape(-1), padding=2)
                out = torch.where(mask, y, out)
    return torch.nn.functional.pixel_shuffle(out, 2)


def pack_upfold(wu, bu, wl, bl, device) -> PackedUpfold:
    """The twelve variants (rs 0..3 x cs 0..2; hat_upfold_* takes W >= 16, so no column is first and last) as bf16 fragments."""
    G, Bd, b0 = upfold_pieces(wu, bu, wl, bl)
    if G.shape[2] != 3 or G.shape[5] != 64:
        raise ValueError(f"hat_upfold is built for 64 -> 3 channels, got {G.shape[5]} -> {G.shape[2]}")
    ws, bs = [], []
    for rs in range(4):
        for cs in range(3):
            F, bias = upfold_variant(G, Bd, b0, rs, cs)
            A = torch.zeros(2, 2, 4, 25, 64, dtype=torch.float64)          # [a][b][m (3: zero)][tap][c]
            A[:, :, :3] = F.permute(1, 2, 0, 4, 5, 3).reshape(2, 2, 3, 25, 64)
            ws.append(frags(A.reshape(16, 25 * 64).to(torch.float32))[0])
            bb = torch.zeros(2, 2, 4, dtype=torch.float64)
            bb[:, :, :3] = bias.permute(1, 2, 0)
            bs.append(bb.reshape(16))
    p = PackedUpfold()
    p.w = torch.stack(ws).to(torch.bfloat16).contiguous().to(device)
    p.bias = torch.stack(bs).to(torch.float32).contiguous().to(device)
    return p


# ------------------------------------------------------------------------------------------------
# hat_vgg_conv (SRVGGNetCompact)
# ------------------------------------------------------------------------------------------------
VGG_NTL = {HAT_BF16: 4, HAT_F32: 2}   # n-tiles of the 64 outputs a workgroup of hat_vgg_conv keeps resident


class PackedVggConv:
    """One conv + activation layer of SRVGGNetCompact for hat_vgg_conv: w [slices][k-steps][n-tiles][64][8] of T, bias and slope fp32[64];
    frame: the layer reads the 3-channel fp32 frame (k = 9 ci + tap) instead of 64-channel rows (k = 64 tap + ci)."""
    __slots__ = ("w", "bias", "slope", "frame", "dtype")


def pack_vgg_conv(weight: torch.Tensor, bias: torch.Tensor, slope: torch.Tensor, dtype: int, device) -> PackedVggConv:
    """weight (64, 64, 3, 3) or (64, 3, 3, 3), bias (64,), slope (64,): the factor on the negative side, per output channel."""
    w = _f32(weight)
    if tuple(w.shape) not in ((64, 64, 3, 3), (64, 3, 3, 3)) or tuple(bias.shape) != (64,) or tuple(slope.shape) != (64,):
        raise ValueError(f"hat_vgg_conv is built for a 3x3 conv of 64 or 3 channels to 64 with 64 slopes, got weight {tuple(w.shape)}, "
                         f"bias {tuple(bias.shape)}, slope {tuple(slope.shape)}")
    p = PackedVggConv()
    p.frame, p.dtype = w.shape[1] == 3, dtype
    m = _pad(w.reshape(64, 27), 64, 32) if p.frame else _tap_major(w)
    ntl = VGG_NTL[dtype]
    f = frags(m)                                                            # [4 n-tiles][k-steps][64][8]
    f = f.reshape(4 // ntl, ntl, f.shape[1], 64, 8).permute(0, 2, 1, 3, 4)   # [slices][k-steps][n-tiles of the slice][64][8]
    p.w = f.to(TORCH_DTYPE[dtype]).contiguous().to(device)
    p.bias, p.slope = _f32(bias).contiguous().to(device), _f32(slope).contiguous().to(device)
    return p


# ------------------------------------------------------------------------------------------------
# hat_rdb_conv (RRDBNet)
# ------------------------------------------------------------------------------------------------
RDB_CIN = (64, 96, 128, 160, 192)   # the five convs of a residual dense block: 32 outputs each, 64 for the last


class PackedRdbConv:
    """One conv of a residual dense block for hat_rdb_conv: w [slices][k-steps][2 n-tiles][64][8] of T with k-step = 9 (channel / 32)
    + tap (1 slice of 32 outputs for convs 1-4, 2 for conv 5), bias fp32[cout]."""
    __slots__ = ("w", "bias", "cin", "cout", "dtype")


def pack_rdb_conv(weight: torch.Tensor, bias: torch.Tensor, dtype: int, device) -> PackedRdbConv:
    """weight (32, cin, 3, 3) with cin in 64, 96, 128, 160, or (64, 192, 3, 3); bias (cout,)."""
    w = _f32(weight)
    cout, cin = (w.shape[0], w.shape[1]) if w.dim() == 4 else (0, 0)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or cin not in RDB_CIN or cout != (64 if cin == 192 else 32) or tuple(bias.shape) != (cout,):
        raise ValueError(f"hat_rdb_conv is built for the 3x3 convs of a residual dense block (64 + 32 k channels to 32, 192 to 64), got weight "
                         f"{tuple(w.shape)}, bias {tuple(bias.shape)}")
    p = PackedRdbConv()
    p.cin, p.cout, p.dtype = cin, cout, dtype
    m = w.reshape(cout, cin // 32, 32, 9).permute(0, 1, 3, 2).reshape(cout, 9 * cin)   # K = (9 (channel / 32) + tap) 32 + channel % 32
    f = frags(m)                                                                      # [cout / 16][k-steps][64][8]
    f = f.reshape(cout // 32, 2, f.shape[1], 64, 8).permute(0, 2, 1, 3, 4)            # [slices][k-steps][2 n-tiles][64][8]
    p.w = f.to(TORCH_DTYPE[dtype]).contiguous().to(device)
    p.bias = _f32(bias).contiguous().to(device)
    return p
