"""Tensor-level wrappers over the C ABI: torch tensors in (device memory, current stream), raw
pointers out.  PyTorch is plumbing here — allocation and stream ownership — no torch op computes
anything on the hot path.  Every wrapper raises if the library is missing or a call fails.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_LRELU, ACT_LRELU02, ACT_NONE, HAT_BF16, HAT_F32, O_FOLD2_NCHW_F32, O_NCHW_F32, O_NHWC_F32, O_NHWC_T, O_PIXSHUF_T,
                   X_NCHW_F32_MEAN, X_NHWC_F32, X_NHWC_T, HatAggrCabDesc, HatCabFoldDesc, HatConvDesc, HatFfnDesc, HatHabTailDesc, HatMlpDesc, HatNafFoldDesc,
                   HatNafHalfDesc, HatEscConvFfnDesc, HatVggConvDesc, HatRdbConvDesc, HatHeadDesc)
# host-side weight packing lives in packing.py; ops.pack_* / ops.Packed* stay the names the engine, the tools and the tests use
from .packing import (ESC_HID_PAD, FP16_SAFE, KC, NAF_WIDTHS, TORCH_DTYPE, PackedConv, PackedEscFfn, PackedFFN, PackedMlp, PackedNafBlock, choose_nt,  # noqa: F401
                      esc_geo_ensemble, pack_esc_convffn, PackedEscRealSkip, ESCFP_HID_PAD, PackedEscFpLk, bicubic_phase_table, escfp_rank1_fold,
                      pack_escfp_convffn, pack_escfp_lk, dysample_fold, pack_escreal_skip, pack_nearest_conv,
                      LTE_HIDDEN, PackedLte, pack_lte,
                      PackedVggConv, pack_vgg_conv,
                      RDB_CIN, PackedRdbConv, pack_rdb_conv,
                      UNI_UPSAMPLERS, PackedEscRealMSkip, conv_nearest_fold, pack_conv_nearest, pack_escrealm_skip, pack_pixshuf_conv, pixshuf_perm,
                      choose_nt_linear, naf_ffn_fold, naf_frags, pack_naf_block,
                      ffn_fp16_range_bound, pack_upfold, pack_cab_squeeze, pack_cab_w2f, pack_conv_weight, pack_ffn, pack_ffn2, pack_ffn3,
                      pack_linear_weight, pack_ocab_mlp, pack_ocab_qkv, pack_pointwise)

DTYPE_CODE = {"f32": HAT_F32, "fp32": HAT_F32, "float32": HAT_F32, "bf16": HAT_BF16, "bfloat16": HAT_BF16}


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("HAT HIP ops need device tensors (no CPU path exists)")
    if not t.is_contiguous():
        raise RuntimeError("HAT HIP ops need contiguous tensors")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-launch timing (bench.py): HIP events on the stream the kernels are enqueued on ----
_prof = None  # None, or a list of (kernel_name, algorithmic_flops, start_event, end_event)


class profile:
    """`with ops.profile() as records:` brackets every kernel launch with HIP events on the current
    stream and records (kernel name as rocprof prints it, algorithmic FLOPs of the launch)."""

    def __enter__(self):
        global _prof
        _prof = []
        return _prof

    def __exit__(self, *exc):
        global _prof
        _prof = None
        return False


def profiling() -> bool:
    return _prof is not None


def _timed(name, flops, fn, tag="", nbytes=0.0):
    """nbytes: ALGORITHMIC HBM bytes of the launch (each operand read once, each result written once)."""
    if _prof is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    _prof.append((name, float(flops), s, e, tag, float(nbytes)))
    return r


_TNAME = {HAT_F32: "float", HAT_BF16: "__bf16"}


def _mean4(mean):
    return (C.c_float * 4)(*[float(mean[i]) if i < len(mean) else 0.0 for i in range(4)])


def _stream16(r1, out, out_mode: int) -> int:
    """HatConvDesc.reserved0 from the tensors' dtypes: bit 0 = r1, bit 1 = the fp32 (O_NHWC_F32) output are FP16 rows (the
    16-bit residual stream; hat_conv / hat_linear accept it on the group conv and the OCAB projection only)."""
    h = 1 if r1 is not None and r1.dtype == torch.float16 else 0
    if out_mode == O_NHWC_F32 and out.dtype == torch.float16:
        h |= 2
    return h


def _sat_ptr(sat: torch.Tensor) -> int:
    """The guard slot of the *_guarded entries: one uint32 (or int32) word of device memory."""
    if sat.dtype not in (torch.uint32, torch.int32) or sat.numel() < 1:
        raise RuntimeError(f"the guard slot is one 32-bit integer word on the device, got {tuple(sat.shape)} {sat.dtype}")
    return _ptr(sat)


def read_sat(word) -> float:
    """The magnitude a guard slot's word stands for: 0.0 for a clean word, else the fp32 value of its bit pattern (inf, nan)."""
    import struct
    return struct.unpack("<f", struct.pack("<I", int(word) & 0xFFFFFFFF))[0]


def conv(pw: PackedConv, x: torch.Tensor, out: torch.Tensor, *, B: int, H: int, W: int, dtype: int, ldx: int, ldo: int,
         x_mode: int = X_NHWC_T, out_mode: int = O_NHWC_T, act: int = ACT_NONE, n_store: Optional[int] = None,
         x0: Optional[torch.Tensor] = None, c_split: int = 0, ldx0: int = 0,
         r1: Optional[torch.Tensor] = None, ldr1: int = 0, r2: Optional[torch.Tensor] = None, ldr2: int = 0,
         r2scale: Optional[torch.Tensor] = None, r2scale_bstride: int = 0, colsum: Optional[torch.Tensor] = None,
         ps_r: int = 0, in_scale: float = 1.0, out_scale: float = 1.0, mean=(0.0, 0.0, 0.0, 0.0), cin: Optional[int] = None,
         ln=None, ln_out: Optional[torch.Tensor] = None, ld_ln: int = 0, gap_out: Optional[torch.Tensor] = None, gap_c: int = 0,
         n16_out: Optional[torch.Tensor] = None, sat: Optional[torch.Tensor] = None):
    """ln=(gamma, beta), ln_out, ld_ln: also emit LayerNorm(result) as T rows from the conv's epilogue (one slice that stores
    every channel), with the per-tile sums of its first gap_c channels (gap_out, conv_tiles blocks) and a compact copy of
    its first 16 channels (n16_out) for the ESC path of the block that consumes it.
    sat: the FP16-range guard's slot (one uint32 on the device): hat_conv_guarded instead of hat_conv, for FP16 output rows only."""
    lib = _lib.load()
    d = HatConvDesc()
    if ln is not None:
        d.ln_g, d.ln_b, d.ln_out, d.ld_ln = _ptr(ln[0]), _ptr(ln[1]), _ptr(ln_out), ld_ln
    if gap_out is not None and gap_c:
        d.gap_out, d.gap_c = _ptr(gap_out), gap_c
    d.n16_out = _ptr(n16_out)
    d.x, d.x0, d.w, d.bias, d.out = _ptr(x), _ptr(x0), _ptr(pw.w), _ptr(pw.bias), _ptr(out)
    d.r1, d.r2, d.r2scale, d.colsum = _ptr(r1), _ptr(r2), _ptr(r2scale), _ptr(colsum)
    d.B, d.H, d.W = B, H, W
    d.Cin, d.ldx, d.x_mode = (pw.cin if cin is None else cin), ldx, x_mode
    d.c_split, d.ldx0 = c_split, ldx0
    d.ksize, d.Kpad, d.nt, d.n_slices, d.w_bstride = pw.ksize, pw.kpad, pw.nt, pw.n_slices, pw.w_bstride
    d.n_store = pw.nout if n_store is None else n_store
    d.ldo, d.out_mode, d.act = ldo, out_mode, act
    d.ldr1, d.ldr2, d.r2scale_bstride, d.ps_r = ldr1, ldr2, r2scale_bstride, ps_r
    d.in_scale, d.out_scale = in_scale, out_scale
    d.mean = _mean4(mean)
    d.dtype = dtype
    d.reserved0 = _stream16(r1, out, out_mode)
    name, flops = "conv_kernel", 0.0
    if _prof is not None:
        wv, pt, tl, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        lib.hat_conv_plan(C.byref(d), C.byref(wv), C.byref(pt), C.byref(tl), C.byref(lds))
        name = f"conv_kernel<{_TNAME[dtype]}, {wv.value}, {pt.value}, {pw.nt}>"
        # algorithmic FLOPs (2*MAC, unpadded).  The 13x13 ESC conv also carries the
        # dynamic depthwise 3x3 that is folded into its weights (2*9*pdim per pixel).
        flops = 2.0 * B * H * W * (pw.ksize ** 2) * d.Cin * pw.nout + (2.0 * 9 * pw.nout * B * H * W if pw.w_bstride else 0.0)
    launch = (lambda: lib.hat_conv(C.byref(d), _stream())) if sat is None else (lambda: lib.hat_conv_guarded(C.byref(d), _sat_ptr(sat), _stream()))
    _timed(name, flops, lambda: _lib.check(launch(), f"hat_conv{'' if sat is None else '_guarded'}(k={pw.ksize}, Cin={d.Cin}, N={pw.nout})"),
           tag=f"k{pw.ksize} {d.Cin}->{pw.nout} {H}x{W} x{x_mode} o{out_mode}{' r1' if r1 is not None else ''}{' r2' if r2 is not None else ''}")


def conv_tiles(pw: PackedConv, H: int, W: int, dtype: int) -> int:
    lib = _lib.load()
    d = HatConvDesc()
    d.B, d.H, d.W, d.Cin, d.ksize, d.nt, d.n_slices, d.dtype = 1, H, W, pw.cin, pw.ksize, pw.nt, pw.n_slices, dtype
    n = C.c_int32(0)
    _lib.check(lib.hat_conv_tiles(C.byref(d), C.byref(n)), "hat_conv_tiles")
    return n.value


def layernorm_blocks() -> int:
    return _lib.load().hat_layernorm_blocks()


def layernorm(x: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, B: int, npix: int, C_: int,
              ldy: int, out_f32: bool, dtype: int, gap: Optional[torch.Tensor] = None, gap_c: int = 0):
    lib = _lib.load()
    _timed("ln_kernel", 0.0, lambda: _lib.check(
        lib.hat_layernorm(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(gap), B, npix, C_, ldy, int(out_f32), gap_c, dtype,
                          _stream()), "hat_layernorm"))


def head_fused_supported(pw: PackedConv, C_: int, gap_c: int, dtype: int) -> bool:
    """hat_head_fused takes conv_first as hat_conv packs it for 3 -> 144 channels (bf16) and pools at most 16 channels."""
    return bool(dtype == HAT_BF16 and C_ == 144 and not pw.frag and pw.ksize == 3 and pw.cin == 3 and pw.nout == 144 and pw.nt == 9
                and pw.n_slices == 1 and pw.kpad >= 96 and gap_c in (0, 4, 8, 12, 16))


def head_fused(pw: PackedConv, x: torch.Tensor, f0: Optional[torch.Tensor], t: torch.Tensor, n: torch.Tensor, ln0, ln1, *, B: int, H: int,
               W: int, ldn: int, dtype: int, in_scale: float = 1.0, mean=(0.0, 0.0, 0.0, 0.0), n16: Optional[torch.Tensor] = None,
               gap: Optional[torch.Tensor] = None, gap_c: int = 0):
    """conv_first + LayerNorm(ln0) + LayerNorm(ln1) in one launch (hat_head_fused): x (B,3,H,W) fp32 -> f0, t (B,H*W,144) fp32,
    n (B,H*W,ldn) bf16, n16 its compact 16-channel copy, gap hat_layernorm's GAP partials of n's first gap_c channels."""
    lib = _lib.load()
    d = HatHeadDesc()
    d.x, d.w, d.bias, d.f0, d.t, d.n, d.n16 = _ptr(x), _ptr(pw.w), _ptr(pw.bias), _ptr(f0), _ptr(t), _ptr(n), _ptr(n16)
    d.ln0_g, d.ln0_b, d.ln1_g, d.ln1_b = _ptr(ln0[0]), _ptr(ln0[1]), _ptr(ln1[0]), _ptr(ln1[1])
    d.gap_partial = _ptr(gap) if gap_c else None
    d.B, d.H, d.W, d.C, d.Kpad, d.ldn, d.gap_c, d.dtype = B, H, W, pw.nout, pw.kpad, ldn, gap_c, dtype
    d.in_scale, d.mean = in_scale, _mean4(mean)
    px = float(B) * H * W
    # bytes: the planes read once; f0 and t (fp32), n (bf16) and its compact copy written once
    _timed("head_fused_kernel", px * (2.0 * 27 * 144 + 2 * 8.0 * 144), lambda: _lib.check(lib.hat_head_fused(C.byref(d), _stream()), "hat_head_fused"),
           tag=f"3->144 {H}x{W} gap{gap_c}", nbytes=px * (12 + (576 if f0 is not None else 0) + 576 + 288 + (32 if n16 is not None else 0)))


def add_f32(a: torch.Tensor, c: torch.Tensor, out: torch.Tensor, *, B: int, n: int, c_bstride: Optional[int] = None):
    """out[b] = a[b] + c[b] (c_bstride = n) or + c (c_bstride = 0: broadcast over the batch); fp32."""
    lib = _lib.load()
    cb = n if c_bstride is None else c_bstride
    _timed("add_f32_kernel", 0.0, lambda: _lib.check(lib.hat_add_f32(_ptr(a), _ptr(c), _ptr(out), B, n, cb, _stream()), "hat_add_f32"))


def rect_sum(x: torch.Tensor, out: torch.Tensor, tmp: torch.Tensor, counter: torch.Tensor, *, B: int, W: int, ld: int, C_: int, r0: int,
             r1: int, c0: int = 0, c1: Optional[int] = None, out_off: int = 0, dtype: Optional[int] = None):
    """out[b][out_off : out_off + C_] = per-channel sums of x (B, rows*W, ld) over rows [r0, r1) x columns [c0, c1) (hat_rect_sum):
    the pooled sums a row band of a sharded frame contributes."""
    lib = _lib.load()
    dt = dtype if dtype is not None else (HAT_BF16 if x.dtype == torch.bfloat16 else HAT_F32)
    o = out.view(B, -1)
    bstride = x.numel() // B
    _timed("rect_sum_kernel", 0.0, lambda: _lib.check(
        lib.hat_rect_sum(_ptr(x), dt, ld, C_, W, r0, r1, c0, (W if c1 is None else c1), bstride, B, o.data_ptr() + 4 * out_off, o.shape[1],
                         _ptr(tmp), _ptr(counter), _stream()), "hat_rect_sum"))


def esc_weights(gap: torch.Tensor, nblk: int, npix: int, w1, b1, w2, b2, plk_packed, w_out, *, B: int, pdim: int,
                ksize: int, kpad: int, dtype: int):
    lib = _lib.load()
    _timed("esc_weights_kernel", 0.0, lambda: _lib.check(
        lib.hat_esc_weights(_ptr(gap), nblk, npix, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(plk_packed), _ptr(w_out), B,
                            pdim, ksize, kpad, dtype, _stream()), "hat_esc_weights"))


def esc_conv13_supported(pdim: int, ksize: int, dtype: int) -> bool:
    return pdim == 16 and ksize == 13 and dtype == HAT_BF16


def esc_conv13(x, wp, y16, *, B: int, H: int, W: int, ldx: int, kpad: int, dtype: int):
    """ESC 13x13 conv on the dedicated kernel (hat_esc_conv13): weights and haloed tile resident in LDS."""
    lib = _lib.load()
    _timed("esc13_kernel", 2.0 * B * H * W * 169 * 256 + 2.0 * 9 * 16 * B * H * W, lambda: _lib.check(
        lib.hat_esc_conv13(_ptr(x), ldx, _ptr(wp), kpad, _ptr(y16), B, H, W, dtype, _stream()), "hat_esc_conv13"),
        tag=f"k13 16->16 {H}x{W} resident")


def eca_scale(colsum, tiles: int, ldc: int, npix: int, wk, k: int, conv_scale: float, tmp, scale, *, B: int, C_: int):
    lib = _lib.load()
    _timed("eca_reduce+scale", 0.0, lambda: _lib.check(
        lib.hat_eca_scale(_ptr(colsum), tiles, ldc, npix, _ptr(wk), k, conv_scale, _ptr(tmp), _ptr(scale), B, C_, _stream()),
        "hat_eca_scale"))


def dwconv_gate(u, wdw, bdw, out, *, B: int, H: int, W: int, hid: int, ldu: int, ldo: int, dtype: int):
    lib = _lib.load()
    _timed(f"dwgate_kernel<{_TNAME[dtype]}>", 2.0 * 9 * 2 * hid * B * H * W, lambda: _lib.check(
        lib.hat_dwconv_gate(_ptr(u), _ptr(wdw), _ptr(bdw), _ptr(out), B, H, W, hid, ldu, ldo, dtype, _stream()),
        "hat_dwconv_gate"))


def ocab_keybias(sal, kv, kb, *, B: int, H: int, W: int, C_: int, ws: int, wse: int, pad: int, k_keep: int, ldsal: int, ldkv: int,
                 dtype: int):
    """HATX focus bias / top-k prune mask per (window, key) (hat_ocab_keybias)."""
    lib = _lib.load()
    _timed("keybias_kernel", 0.0, lambda: _lib.check(
        lib.hat_ocab_keybias(_ptr(sal), ldsal, _ptr(kv), ldkv, _ptr(kb), B, H, W, C_, ws, wse, pad, k_keep, dtype, _stream()), "hat_ocab_keybias"))


def ocab_attention_kb(q, kv, bias_rot, kb, out, *, B: int, H: int, W: int, C_: int, heads: int, ws: int, wse: int, pad: int, ldq: int,
                      ldkv: int, ldo: int, dtype: int):
    lib = _lib.load()
    _timed(f"ocab_attn_kernel<{_TNAME[dtype]}, kb>", 2.0 * 2 * wse * wse * C_ * B * H * W, lambda: _lib.check(
        lib.hat_ocab_attention_kb(_ptr(q), _ptr(kv), _ptr(bias_rot), _ptr(kb), _ptr(out), B, H, W, C_, heads, ws, wse, pad, ldq, ldkv, ldo,
                                  dtype, _stream()), "hat_ocab_attention_kb"))


def ocab_mlp_supported(C_: int, hidden: int, dtype: int) -> bool:
    return C_ == 144 and hidden == 288 and dtype == HAT_BF16


def ocab_qkv(pm: PackedMlp, x, out, *, B: int, H: int, W: int, ldx: int, ldo: int, dtype: int):
    """out rows [q | k | v] (432 channels) = both OCAB projections of x in one launch (hat_ocab_qkv)."""
    lib = _lib.load()
    d = HatMlpDesc()
    d.x, d.w1f, d.b1, d.out = _ptr(x), _ptr(pm.w1f), _ptr(pm.b1), _ptr(out)
    d.B, d.H, d.W, d.C, d.hidden, d.ldx, d.ldo, d.dtype = B, H, W, pm.C, pm.hidden, ldx, ldo, dtype
    _timed("ocab_qkv_kernel", 2.0 * pm.C * pm.hidden * B * H * W, lambda: _lib.check(lib.hat_ocab_qkv(C.byref(d), _stream()), "hat_ocab_qkv"),
           tag=f"qkv {pm.C}->{pm.hidden} {H}x{W}", nbytes=float(B * H * W) * 2 * (ldx + pm.hidden))


def ocab_mlp(pm: PackedMlp, x, r1, out, *, B: int, H: int, W: int, ldx: int, ldr1: int, ldo: int, out_f32: bool, dtype: int):
    """out = r1 + fc2(GELU(fc1(x))) in one launch (hat_ocab_mlp): the 288-wide hidden tensor never reaches HBM.
    r1 may be FP16 rows (the 16-bit residual stream) when out is T rows."""
    lib = _lib.load()
    d = HatMlpDesc()
    d.x, d.w1f, d.b1, d.w2f, d.b2, d.r1, d.out = _ptr(x), _ptr(pm.w1f), _ptr(pm.b1), _ptr(pm.w2f), _ptr(pm.b2), _ptr(r1), _ptr(out)
    r16 = r1.dtype == torch.float16
    d.B, d.H, d.W, d.C, d.hidden, d.ldx, d.ldr1, d.ldo, d.dtype = B, H, W, pm.C, pm.hidden, ldx, ldr1, ldo, dtype
    d.out_f32 = int(out_f32) | (2 if r16 else 0)
    _timed(f"ocab_mlp_kernel<{'true' if out_f32 else 'false'}>", 2.0 * 2 * pm.C * pm.hidden * B * H * W,
           lambda: _lib.check(lib.hat_ocab_mlp(C.byref(d), _stream()), "hat_ocab_mlp"),
           tag=f"mlp {pm.C}->{pm.hidden}->{pm.C} {H}x{W}",
           nbytes=float(B * H * W) * (2 * ldx + (2 if r16 else 4) * pm.C + (4 if out_f32 else 2) * pm.C))


def sgfn_gate(u, wdw, bdw, out, *, B: int, H: int, W: int, half: int, ldu: int, ldo: int, dtype: int):
    """HATX SGFN: out = [dw3x3(u[:half]) * silu(u[half:]) | u[half:]] (hat_sgfn_gate)."""
    lib = _lib.load()
    _timed(f"sgfn_gate_kernel<{_TNAME[dtype]}>", 2.0 * 9 * half * B * H * W, lambda: _lib.check(
        lib.hat_sgfn_gate(_ptr(u), _ptr(wdw), _ptr(bdw), _ptr(out), B, H, W, half, ldu, ldo, dtype, _stream()), "hat_sgfn_gate"))


# ------------------------------------------------------------------------------------------------
# the NAF stem of HybridHATNAF (hat_naf_half / hat_naf_fold)
# ------------------------------------------------------------------------------------------------
def naf_tiles(H: int, W: int) -> int:
    """Tiles per sample of hat_naf_half = slots per sample of its pool partials."""
    n = _lib.load().hat_naf_half_tiles(H, W)
    _lib.check(min(n, 0), "hat_naf_half_tiles")
    return n


def naf_half(r_in, g_out, w1, b1, dww, dwb, *, B: int, H: int, W: int, C_: int, dtype: int, ldr: Optional[int] = None, ldo: Optional[int] = None,
             gprev=None, ldg: Optional[int] = None, wf=None, wf_bstride: int = 0, bf=None, bf_bstride: int = 0, r_out=None, partials=None):
    """One half of a NAFBlock (hat_naf_half): g_out = gate(dw3x3(W1 r + b1)) with r = r_in (form a) or, with gprev / wf / bf /
    r_out, r = r_in + Wf gprev + bf, also written to r_out (form b).  w1 None (form b): only r_out, the stem's last projection.
    partials: the (B, naf_tiles, C_) fp32 pool partials of g_out."""
    lib = _lib.load()
    d = HatNafHalfDesc()
    d.r_in, d.gprev, d.wf, d.bf, d.r_out = _ptr(r_in), _ptr(gprev), _ptr(wf), _ptr(bf), _ptr(r_out)
    d.w1, d.b1, d.dww, d.dwb, d.g_out, d.partials = _ptr(w1), _ptr(b1), _ptr(dww), _ptr(dwb), _ptr(g_out), _ptr(partials)
    d.wf_bstride, d.bf_bstride = wf_bstride, bf_bstride
    d.B, d.H, d.W, d.C, d.dtype = B, H, W, C_, dtype
    d.ldr, d.ldg, d.ldo = (C_ if ldr is None else ldr), (C_ if ldg is None else ldg), (C_ if ldo is None else ldo)
    form = "a" if gprev is None else ("b" if w1 is not None else "proj")
    es, npx = (2 if dtype == HAT_BF16 else 4), float(B * H * W)
    flops = 2.0 * npx * C_ * ((2 * C_ if w1 is not None else 0) + (C_ if gprev is not None else 0)) + (2.0 * 9 * 2 * C_ * npx if w1 is not None else 0.0)
    nbytes = npx * C_ * (4 + (4 + es if gprev is not None else 0) + (es if w1 is not None else 0))
    _timed(f"naf_half_kernel<{_TNAME[dtype]}, {C_}>", flops, lambda: _lib.check(lib.hat_naf_half(C.byref(d), _stream()), f"hat_naf_half(c={C_}, form {form})"),
           tag=f"naf {form} c{C_} {H}x{W}{' pool' if partials is not None else ''}", nbytes=nbytes)


def naf_fold(partials, blk: PackedNafBlock, wf, bf, *, B: int, H: int, W: int, C_: int, dtype: int):
    """The SCA of a NAFBlock folded into its pw2 (hat_naf_fold): wf (B, C_ * C_) T fragments, bf (B, C_) fp32 for naf_half."""
    lib = _lib.load()
    d = HatNafFoldDesc()
    d.partials, d.wsca, d.bsca, d.w2, d.b2, d.beta = _ptr(partials), _ptr(blk.wsca), _ptr(blk.bsca), _ptr(blk.w2), _ptr(blk.b2), _ptr(blk.beta)
    d.wf, d.bf, d.npix, d.B, d.tiles, d.C, d.dtype = _ptr(wf), _ptr(bf), H * W, B, naf_tiles(H, W), C_, dtype
    _timed(f"naf_fold_kernel<{_TNAME[dtype]}, {C_}>", 0.0, lambda: _lib.check(lib.hat_naf_fold(C.byref(d), _stream()), f"hat_naf_fold(c={C_})"),
           tag=f"naf fold c{C_} {H}x{W}")


# ------------------------------------------------------------------------------------------------
# ESC (hat_esc_convffn / hat_window_attention_r / hat_esc_layernorm / hat_esc_shuffle_add)
# ------------------------------------------------------------------------------------------------
def esc_convffn_tiles(H: int, W: int) -> int:
    """Tiles per sample of hat_esc_convffn = slots per sample of its pool partials."""
    n = _lib.load().hat_esc_convffn_tiles(H, W)
    _lib.check(min(n, 0), "hat_esc_convffn_tiles")
    return n


def _esc_convffn(C_: int, entry: str, pf: PackedEscFfn, x, out, *, B: int, H: int, W: int, dtype: int, ldx: int, ldr: int, ldo: int, ln=None,
             eps: float = 1e-6, r=None, partials=None):
    """esc_convffn_kernel at C_ channels through `entry` (hat_esc_convffn: 64, hat_escfp_convffn: 48); the **kw of the public names."""
    lib = _lib.load()
    d = HatEscConvFfnDesc()
    d.x, d.w1, d.b1, d.dww, d.dwb, d.w2, d.b2 = _ptr(x), _ptr(pf.w1), _ptr(pf.b1), _ptr(pf.dww), _ptr(pf.dwb), _ptr(pf.w2), _ptr(pf.b2)
    if ln is not None:
        d.ln_g, d.ln_b = _ptr(ln[0]), _ptr(ln[1])
    d.ln_eps = eps
    d.r, d.out, d.partials = _ptr(r), _ptr(out), _ptr(partials)
    d.B, d.H, d.W, d.hid_p, d.ldx, d.ldr, d.ldo, d.dtype = B, H, W, pf.hid_p, ldx, ldr, ldo, dtype
    d.out_f32 = int(out.dtype == torch.float32)
    es, npx = (4 if d.out_f32 or dtype == HAT_F32 else 2), float(B * H * W)
    _timed(f"esc_convffn_kernel<{_TNAME[dtype]}, {C_}, {pf.hid_p}>", 2.0 * npx * pf.hid * (2 * C_ + 9),
           lambda: _lib.check(getattr(lib, entry)(C.byref(d), _stream()), f"{entry}(hid={pf.hid})"),
           tag=f"convffn {C_}->{pf.hid}->{C_} {H}x{W}{' ln' if ln is not None else ''}{' r' if r is not None else ''}{' pool' if partials is not None else ''}",
           nbytes=npx * C_ * (4 + es + (4 if r is not None else 0)))


def esc_convffn(pf: PackedEscFfn, x, out, *, ldx: int = 64, ldr: int = 64, ldo: int = 64, **kw):
    """out = ConvFFN(ln ? LayerNorm(x; ln = (gamma, beta), eps) : x) (+ r) in one launch (hat_esc_convffn).  x, r: fp32 rows; out: fp32
    rows when it is an fp32 tensor, else T rows; partials: the (B, esc_convffn_tiles, 16) fp32 pool partials of out[..., :16]."""
    _esc_convffn(64, "hat_esc_convffn", pf, x, out, ldx=ldx, ldr=ldr, ldo=ldo, **kw)


def window_attention_r(q, kv, bias, out, *, B: int, h: int, w: int, C_: int, heads: int, ws: int, ldq: int, ldkv: int, ldo: int, dtype: int):
    """ESC's 32 x 32 window attention with reflected edge windows (hat_window_attention_r; esc_arch.py:205-250); q pre-scaled."""
    lib = _lib.load()
    nw = -(-h // ws) * -(-w // ws)
    _timed(f"window_attention_r_kernel<{_TNAME[dtype]}>", 2.0 * 2 * (ws * ws) ** 2 * C_ * B * nw, lambda: _lib.check(
        lib.hat_window_attention_r(_ptr(q), _ptr(kv), _ptr(bias), _ptr(out), B, h, w, C_, heads, ws, ldq, ldkv, ldo, dtype, _stream()),
        "hat_window_attention_r"), tag=f"attn ws{ws} {h}x{w}")


def _esc_layernorm(C_: int, entry: str, x, y, gamma, beta, *, npix: int, dtype: int, ldx: int, ldy: int, eps: float = 1e-6):
    lib = _lib.load()
    _timed(f"esc_layernorm_kernel<{_TNAME[dtype]}, {C_}>", 0.0, lambda: _lib.check(
        getattr(lib, entry)(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), eps, npix, ldx, ldy, dtype, _stream()), entry),
        tag=f"ln{C_} eps")


def esc_layernorm(x, y, gamma, beta, *, ldx: int = 64, ldy: int = 64, **kw):
    """y (T rows) = LayerNorm over 64 channels of x (fp32 rows) with `eps` (hat_esc_layernorm)."""
    _esc_layernorm(64, "hat_esc_layernorm", x, y, gamma, beta, ldx=ldx, ldy=ldy, **kw)


def esc_shuffle_add(rows, x, y, *, B: int, H: int, W: int, s: int, ld: int):
    """y (B,3,sH,sW) = pixel_shuffle(rows (B,H,W,ld) fp32) + repeat_interleave(x (B,3,H,W), s*s) (hat_esc_shuffle_add)."""
    lib = _lib.load()
    _timed("esc_shuffle_add_kernel", 0.0, lambda: _lib.check(
        lib.hat_esc_shuffle_add(_ptr(rows), _ptr(x), _ptr(y), B, H, W, s, ld, _stream()), "hat_esc_shuffle_add"), tag=f"shuffle x{s} {H}x{W}")


# ------------------------------------------------------------------------------------------------
# ESCReal (hat_escreal_skip / hat_dysample)
# ------------------------------------------------------------------------------------------------
def escreal_skip(ps: PackedEscRealSkip, x, out, *, B: int, H: int, W: int, dtype: int, r=None, ldr: int = 64, ldo: int = 64):
    """out (fp32 rows) = [r +] skip(x), x (B,3,H,W) fp32 planes: the reflect-padded 7x7 skip branch of ESCReal in one launch."""
    lib = _lib.load()
    npx = float(B * H * W)
    _timed(f"escreal_skip_kernel<{_TNAME[dtype]}>", 2.0 * npx * 128 * (147 + 64), lambda: _lib.check(
        lib.hat_escreal_skip(_ptr(x), _ptr(ps.w1), _ptr(ps.b1), _ptr(ps.w3), _ptr(ps.b3), _ptr(r), _ptr(out), B, H, W, ldr, ldo, dtype,
                             _stream()), "hat_escreal_skip"),
        tag=f"skip 3->128->64 {H}x{W}{' r' if r is not None else ''}", nbytes=npx * (12 + 256 + (256 if r is not None else 0)))


def dysample(rows, init_pos, bias, y, *, B: int, H: int, W: int, s: int, ld: int):
    """y (B,3,sH,sW) fp32 = DySample's gather over rows (B,H*W,ld) fp32 = [offset | scope | 12 projected values] (hat_dysample)."""
    lib = _lib.load()
    _timed("dysample_kernel", 0.0, lambda: _lib.check(
        lib.hat_dysample(_ptr(rows), _ptr(init_pos), _ptr(bias), _ptr(y), B, H, W, s, ld, _stream()), "hat_dysample"),
        tag=f"dysample x{s} {H}x{W}", nbytes=4.0 * B * H * W * (ld + 3 * s * s))


# ------------------------------------------------------------------------------------------------
# ESCRealM (hat_unshuffle_pad / hat_escrealm_skip / hat_shuffle_planes)
# ------------------------------------------------------------------------------------------------
def unshuffle_pad(x, rows, *, B: int, h: int, w: int, f: int, ld: int):
    """rows (B, ceil(h/f) * ceil(w/f), ld) fp32 = PixelUnshuffle(f) of x (B,3,h,w) reflect-padded right / bottom to a multiple of f."""
    lib = _lib.load()
    _timed("unshuffle_pad_kernel", 0.0, lambda: _lib.check(
        lib.hat_unshuffle_pad(_ptr(x), _ptr(rows), B, h, w, f, ld, _stream()), "hat_unshuffle_pad"),
        tag=f"unshuffle /{f} {h}x{w}", nbytes=4.0 * B * 3 * (h * w + f * f * (-(-h // f)) * (-(-w // f))))


def escrealm_skip(ps: PackedEscRealMSkip, x, out, *, B: int, H: int, W: int, dtype: int, ldx: int, r=None, ldr: int = 64, ldo: int = 64):
    """out (fp32 rows) = [r +] skip(x), x (B,H*W,ldx) fp32 rows of 12 or 48 unshuffled channels (hat_escrealm_skip)."""
    lib = _lib.load()
    npx = float(B * H * W)
    _timed(f"escrealm_skip_kernel<{_TNAME[dtype]}, {ps.cin}>", 2.0 * npx * 128 * (ps.cin + 49 + 64), lambda: _lib.check(
        lib.hat_escrealm_skip(_ptr(x), _ptr(ps.w0), _ptr(ps.b0), _ptr(ps.dw), _ptr(ps.bdw), _ptr(ps.w3), _ptr(ps.b3), _ptr(r), _ptr(out),
                              B, H, W, ps.cin, ldx, ldr, ldo, dtype, _stream()), "hat_escrealm_skip"),
        tag=f"skip {ps.cin}->128->64 {H}x{W}{' r' if r is not None else ''}", nbytes=npx * (4 * ps.cin + 256 + (256 if r is not None else 0)))


def shuffle_planes(rows, y, *, B: int, H: int, W: int, s: int, ld: int):
    """y (B,3,sH,sW) fp32 = pixel_shuffle(rows (B,H,W,ld) fp32, s) (hat_shuffle_planes)."""
    lib = _lib.load()
    _timed("shuffle_planes_kernel", 0.0, lambda: _lib.check(
        lib.hat_shuffle_planes(_ptr(rows), _ptr(y), B, H, W, s, ld, _stream()), "hat_shuffle_planes"),
        tag=f"shuffle x{s} {H}x{W}", nbytes=4.0 * B * H * W * (ld + 3 * s * s))


def _shuffle_src(what: str, rows, base, B: int, H: int, W: int, s: int, ld: int):
    """The checks shuffle_to_u8 / shuffle_to_yuv make of their source: rows (B,H,W,ld) fp32, base None or (B,3,H,W) fp32 planes."""
    if not isinstance(s, int) or isinstance(s, bool) or not 1 <= s <= 8:
        raise RuntimeError(f"{what}: the shuffle factor is 1..8, got {s!r}")
    if rows.dtype != torch.float32 or not rows.is_cuda or not rows.is_contiguous() or ld < 3 * s * s or rows.numel() != B * H * W * ld:
        raise RuntimeError(f"{what} needs contiguous ({B},{H},{W},ld >= {3 * s * s}) fp32 device rows, got {tuple(rows.shape)} {rows.dtype} for ld {ld}")
    if base is not None and (base.dtype != torch.float32 or tuple(base.shape) != (B, 3, H, W) or not base.is_contiguous() or base.device != rows.device):
        raise RuntimeError(f"{what} needs a contiguous ({B},3,{H},{W}) fp32 base image on {rows.device}, got {tuple(base.shape)} {base.dtype} "
                           f"on {base.device}")


def shuffle_to_u8(rows, base, dst, *, B: int, H: int, W: int, s: int, ld: int, bgr: bool = False):
    """dst (B,h_out,w_out,3) uint8 (rows may be pitched) = planes_to_u8 of what esc_shuffle_add (base (B,3,H,W)) or shuffle_planes
    (base None) writes for rows (B,H,W,ld) fp32, cropped to the top-left h_out x w_out pixels; no fp32 image is written
    (hat_shuffle_to_u8)."""
    lib = _lib.load()
    _shuffle_src("shuffle_to_u8", rows, base, B, H, W, s, ld)
    if dst.dtype != torch.uint8 or not dst.is_cuda or dst.dim() != 4 or dst.shape[0] != B or dst.shape[3] != 3 or dst.stride(-1) != 1 \
            or dst.stride(-2) != 3 or dst.shape[1] > s * H or dst.shape[2] > s * W or dst.device != rows.device:
        raise RuntimeError(f"shuffle_to_u8 needs a ({B},h_out <= {s * H},w_out <= {s * W},3) uint8 destination on {rows.device} with interleaved "
                           f"pixels, got {tuple(dst.shape)} {dst.dtype} on {dst.device}")
    _timed("shuffle_to_u8_kernel", 0.0, lambda: _lib.check(
        lib.hat_shuffle_to_u8(_ptr(rows), ld, _ptr(base), B, H, W, s, dst.data_ptr(), dst.stride(1), dst.stride(0), dst.shape[1], dst.shape[2],
                              int(bool(bgr)), _stream()), "hat_shuffle_to_u8"),
        tag=f"shuffle x{s} {H}x{W} -> u8 {dst.shape[1]}x{dst.shape[2]}", nbytes=B * (4.0 * H * W * (ld + (3 if base is not None else 0))
                                                                                   + 3.0 * dst.shape[1] * dst.shape[2]))


def shuffle_to_yuv(rows, base, y, cb, cr, from_rgb, *, B: int, H: int, W: int, s: int, ld: int, sub, depth: int = 8, msb=False):
    """The views Y (B,h_out,w_out), Cb, Cr of any subsampling (None, None and sub=None: grey), centre-sited = planes_to_yuv of what
    esc_shuffle_add / shuffle_planes writes for rows (and base), cropped to the views' size; no fp32 image is written
    (hat_shuffle_to_yuv)."""
    lib = _lib.load()
    _shuffle_src("shuffle_to_yuv", rows, base, B, H, W, s, ld)
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="shuffle_to_yuv")
    if y.shape[0] != B or y.shape[1] > s * H or y.shape[2] > s * W or y.device != rows.device:
        raise RuntimeError(f"shuffle_to_yuv needs a ({B},h_out <= {s * H},w_out <= {s * W}) Y view on {rows.device}, got {tuple(y.shape)} on {y.device}")
    m, name = _f12(from_rgb), _sub_name(sub, depth)
    _timed(f"shuffle_to_yuv_kernel<{name}>", 0.0, lambda: _lib.check(
        lib.hat_shuffle_to_yuv(_ptr(rows), ld, _ptr(base), B, H, W, s, C.byref(surf), y.shape[1], y.shape[2], m, _stream()), "hat_shuffle_to_yuv"),
        tag=f"shuffle x{s} {H}x{W} -> {name} {y.shape[1]}x{y.shape[2]}", nbytes=B * (4.0 * H * W * (ld + (3 if base is not None else 0))
                                                                                    + 3.0 * y.shape[1] * y.shape[2]))


# ------------------------------------------------------------------------------------------------
# SRVGGNetCompact (hat_vgg_conv)
# ------------------------------------------------------------------------------------------------
def vgg_conv(pv: PackedVggConv, x, out, *, B: int, H: int, W: int, dtype: int, ldx: int = 64, ldo: int = 64):
    """out (B,H,W,ldo) T rows = PReLU-like(conv3x3(x) + bias) with pv.slope on the negative side (hat_vgg_conv): x (B,H,W,ldx) T rows
    of 64 channels, or, for a layer packed from a 3-channel weight, the (B,3,H,W) fp32 frame."""
    lib = _lib.load()
    if pv.dtype != dtype:
        raise RuntimeError(f"vgg_conv: the layer is packed for dtype {pv.dtype}, the launch asks for {dtype}")
    d = HatVggConvDesc()
    d.x, d.w, d.bias, d.slope, d.out = _ptr(x), _ptr(pv.w), _ptr(pv.bias), _ptr(pv.slope), _ptr(out)
    d.B, d.H, d.W, d.ldx, d.ldo, d.frame, d.dtype = B, H, W, (0 if pv.frame else ldx), ldo, int(pv.frame), dtype
    npx, es, cin = float(B * H * W), (2 if dtype == HAT_BF16 else 4), (3 if pv.frame else 64)
    _timed(f"vgg_conv_kernel<{_TNAME[dtype]}, {'true' if pv.frame else 'false'}>", 2.0 * npx * 9 * cin * 64,
           lambda: _lib.check(lib.hat_vgg_conv(C.byref(d), _stream()), "hat_vgg_conv"),
           tag=f"vgg {cin}->64 {H}x{W}", nbytes=npx * ((12 if pv.frame else 64 * es) + 64 * es))


def vgg_conv_tiles(B: int, H: int, W: int, dtype: int):
    """-> (tiles, workgroups per slice, slices) of a hat_vgg_conv launch: workgroup i < min(workgroups, tiles) of a slice takes the
    tiles i, i + workgroups, ... (hat_vgg_conv_tiles)."""
    lib = _lib.load()
    t, g, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib.hat_vgg_conv_tiles(B, H, W, dtype, C.byref(t), C.byref(g), C.byref(s)), "hat_vgg_conv_tiles")
    return t.value, g.value, s.value


# ------------------------------------------------------------------------------------------------
# RRDBNet (hat_rdb_conv)
# ------------------------------------------------------------------------------------------------
def rdb_conv(pr: PackedRdbConv, x, out, *, B: int, H: int, W: int, dtype: int, ldx: int, ldo: int, out_off: int, slope: float = 0.2,
             beta1: float = 1.0, beta2: float = 1.0, r1=None, r2=None, s_out=None):
    """One conv of a residual dense block on dense rows (hat_rdb_conv).  Convs 1-4: out[..., out_off : out_off + 32] = lrelu_slope(conv(x[...,
    :cin]) + bias), out may be x (out_off = cin).  Conv 5 (cin 192): v = beta1 (conv + bias) + r1, then beta2 v + r2 when r2 is given; s_out
    (B, H W, 64) fp32 = v and out[..., out_off : out_off + 64] = v rounded to T.  r1, r2: fp32 rows of 64."""
    lib = _lib.load()
    if pr.dtype != dtype:
        raise RuntimeError(f"rdb_conv: the layer is packed for dtype {pr.dtype}, the launch asks for {dtype}")
    d = HatRdbConvDesc()
    d.x, d.w, d.bias, d.out, d.r1, d.r2, d.s_out = _ptr(x), _ptr(pr.w), _ptr(pr.bias), _ptr(out), _ptr(r1), _ptr(r2), _ptr(s_out)
    d.B, d.H, d.W, d.cin, d.cout, d.ldx, d.ldo, d.out_off = B, H, W, pr.cin, pr.cout, ldx, ldo, out_off
    d.slope, d.beta1, d.beta2, d.dtype = slope, beta1, beta2, dtype
    npx, es = float(B * H * W), (2 if dtype == HAT_BF16 else 4)
    nres = (r1 is not None) + (r2 is not None) + (s_out is not None)
    _timed(f"rdb_conv_kernel<{pr.cin}>", 2.0 * npx * 9 * pr.cin * pr.cout, lambda: _lib.check(lib.hat_rdb_conv(C.byref(d), _stream()), "hat_rdb_conv"),
           tag=f"rdb {pr.cin}->{pr.cout} {H}x{W}", nbytes=npx * ((pr.cin + pr.cout) * es + 256.0 * nres))


def rdb_conv_tiles(B: int, H: int, W: int, cin: int):
    """-> (tiles, workgroups per slice, slices) of a hat_rdb_conv launch: workgroup i < min(workgroups, tiles) of a slice takes the
    tiles i, i + workgroups, ... (hat_rdb_conv_tiles)."""
    lib = _lib.load()
    t, g, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib.hat_rdb_conv_tiles(B, H, W, cin, C.byref(t), C.byref(g), C.byref(s)), "hat_rdb_conv_tiles")
    return t.value, g.value, s.value


# ------------------------------------------------------------------------------------------------
# ESCFP (hat_escfp_convffn / hat_escfp_layernorm / hat_escfp_weights / hat_escfp_shuffle_bicubic)
# ------------------------------------------------------------------------------------------------
def escfp_convffn(pf: PackedEscFfn, x, out, *, ldx: int = 48, ldr: int = 48, ldo: int = 48, **kw):
    """esc_convffn at 48 channels (hat_escfp_convffn); pf from pack_escfp_convffn."""
    _esc_convffn(48, "hat_escfp_convffn", pf, x, out, ldx=ldx, ldr=ldr, ldo=ldo, **kw)


def escfp_layernorm(x, y, gamma, beta, *, ldx: int = 48, ldy: int = 48, **kw):
    """y (T rows) = LayerNorm over 48 channels of x (fp32 rows) with `eps` (hat_escfp_layernorm)."""
    _esc_layernorm(48, "hat_escfp_layernorm", x, y, gamma, beta, ldx=ldx, ldy=ldy, **kw)


def escfp_weights(partials, nblk: int, npix: int, lk: PackedEscFpLk, w_out, *, B: int, dtype: int):
    """w_out (B,16,lk.kpad) T = the dense rank-1 weights of the decomposed large-kernel branch from the pool partials (hat_escfp_weights)."""
    lib = _lib.load()
    _timed("escfp_weights_kernel", 0.0, lambda: _lib.check(
        lib.hat_escfp_weights(_ptr(partials), nblk, npix, _ptr(lk.w1), _ptr(lk.b1), _ptr(lk.w2), _ptr(lk.b2), _ptr(lk.lk_channel),
                              _ptr(lk.lk_spatial), _ptr(w_out), B, lk.kpad, dtype, _stream()), "hat_escfp_weights"))


def escfp_shuffle_bicubic(rows, x, ptab, y, *, B: int, H: int, W: int, s: int, ld: int):
    """y (B,3,sH,sW) = pixel_shuffle(rows (B,H,W,ld) fp32) + bicubic x`s` of x (B,3,H,W); ptab = bicubic_phase_table(s) on the device."""
    lib = _lib.load()
    _timed("escfp_shuffle_bicubic_kernel", 0.0, lambda: _lib.check(
        lib.hat_escfp_shuffle_bicubic(_ptr(rows), _ptr(x), _ptr(ptab), _ptr(y), B, H, W, s, ld, _stream()), "hat_escfp_shuffle_bicubic"),
        tag=f"shuffle+bicubic x{s} {H}x{W}", nbytes=4.0 * B * H * W * (ld + 3 + 3 * s * s))


# ------------------------------------------------------------------------------------------------
# ESC-LTE (hat_lte_query)
# ------------------------------------------------------------------------------------------------
LTE_TILE = 32   # queries per workgroup of hat_lte_query


def lte_query(pl: PackedLte, coef, freq, inp, out, *, H: int, W: int, ldc: int, ldf: int, dtype: int, coord=None, cell=None,
              grid=None, cell_yx=(0.0, 0.0), out_affine=(1.0, 0.0)):
    """The LTE head on the rows coef / freq (H*W, ld) fp32 of a feature map and the normalised input inp (3,H,W) (hat_lte_query).
    Explicit mode: coord, cell (Q,2) fp32 -> out (Q,3).  Grid mode: grid=(h, w), cell_yx the one cell -> out (3,h,w) planes.
    out_affine=(a, b): out * a + b."""
    lib = _lib.load()
    if (coord is None) == (grid is None) or (coord is None) != (cell is None):
        raise ValueError("lte_query takes either coord and cell or grid")
    if coord is not None:
        Q, gh, gw = int(coord.shape[0]), 0, 0
        if tuple(coord.shape) != (Q, 2) or tuple(cell.shape) != (Q, 2) or coord.dtype != torch.float32 or cell.dtype != torch.float32:
            raise ValueError(f"lte_query expects coord and cell as (Q,2) fp32, got {tuple(coord.shape)} {coord.dtype} and {tuple(cell.shape)} {cell.dtype}")
        if out.numel() != 3 * Q:
            raise ValueError(f"lte_query: out holds {out.numel()} values, {Q} queries need {3 * Q}")
    else:
        gh, gw = int(grid[0]), int(grid[1])
        Q = gh * gw
        if out.numel() != 3 * Q:
            raise ValueError(f"lte_query: out holds {out.numel()} values, a {gh}x{gw} grid needs {3 * Q}")
    if out.dtype != torch.float32 or coef.dtype != torch.float32 or freq.dtype != torch.float32 or inp.dtype != torch.float32:
        raise ValueError("lte_query expects fp32 coef / freq rows, fp32 input planes and an fp32 output")
    if coef.numel() < (H * W - 1) * ldc + LTE_HIDDEN or freq.numel() < (H * W - 1) * ldf + LTE_HIDDEN or inp.numel() != 3 * H * W:
        raise ValueError(f"lte_query: coef / freq / inp do not hold a {H}x{W} map")
    hd = float(LTE_HIDDEN)
    flops = Q * (4.0 * (2.0 * hd * hd * 3 + 2.0 * hd * 3 + 5.0 * hd) + 30.0)
    wbytes = 3 * hd * hd * (2 if dtype == HAT_BF16 else 4)
    nbytes = 4.0 * (min(4 * Q, H * W) * 2 * hd + 3 * H * W + 3 * Q + (4 * Q if coord is not None else 0)) + wbytes
    _timed(f"lte_query_kernel<{_TNAME[dtype]}>", flops, lambda: _lib.check(
        lib.hat_lte_query(_ptr(coef), _ptr(freq), ldc, ldf, _ptr(inp), H, W, _ptr(pl.phase), _ptr(pl.w[0]), _ptr(pl.b[0]), _ptr(pl.w[1]),
                          _ptr(pl.b[1]), _ptr(pl.w[2]), _ptr(pl.b[2]), _ptr(pl.w4), _ptr(pl.b4), _ptr(coord), _ptr(cell), Q, gh, gw,
                          float(cell_yx[0]), float(cell_yx[1]), float(out_affine[0]), float(out_affine[1]), _ptr(out), dtype, _stream()),
        "hat_lte_query"), tag=f"lte {'grid ' + str(gh) + 'x' + str(gw) if coord is None else 'Q=' + str(Q)} on {H}x{W}", nbytes=nbytes)


def _lte_grid_args(what: str, pl: PackedLte, coef, freq, inp, H: int, W: int, ldc: int, ldf: int, grid, cell_yx, out_affine):
    """What lte_query_u8 / lte_query_yuv pass ahead of their sink: the checks of lte_query's grid mode, then (the C arguments up to
    out_b, the flops and the bytes of the launch without its stores)."""
    gh, gw = int(grid[0]), int(grid[1])
    if coef.dtype != torch.float32 or freq.dtype != torch.float32 or inp.dtype != torch.float32:
        raise ValueError(f"{what} expects fp32 coef / freq rows and fp32 input planes")
    if coef.numel() < (H * W - 1) * ldc + LTE_HIDDEN or freq.numel() < (H * W - 1) * ldf + LTE_HIDDEN or inp.numel() != 3 * H * W:
        raise ValueError(f"{what}: coef / freq / inp do not hold a {H}x{W} map")
    Q, hd = gh * gw, float(LTE_HIDDEN)
    flops = Q * (4.0 * (2.0 * hd * hd * 3 + 2.0 * hd * 3 + 5.0 * hd) + 30.0)
    nbytes = 4.0 * (min(4 * Q, H * W) * 2 * hd + 3 * H * W) + 3 * hd * hd * (2 if pl.w[0].element_size() == 2 else 4)
    args = (_ptr(coef), _ptr(freq), ldc, ldf, _ptr(inp), H, W, _ptr(pl.phase), _ptr(pl.w[0]), _ptr(pl.b[0]), _ptr(pl.w[1]), _ptr(pl.b[1]),
            _ptr(pl.w[2]), _ptr(pl.b[2]), _ptr(pl.w4), _ptr(pl.b4), gh, gw, float(cell_yx[0]), float(cell_yx[1]), float(out_affine[0]),
            float(out_affine[1]))
    return args, flops, nbytes


def lte_query_u8(pl: PackedLte, coef, freq, inp, out, *, H: int, W: int, ldc: int, ldf: int, dtype: int, grid, cell_yx=(0.0, 0.0),
                 out_affine=(1.0, 0.0), bgr: bool = False):
    """lte_query's grid mode ending in bytes: out (h, w, 3) or (1, h, w, 3) uint8 with interleaved pixels (rows may be pitched) =
    planes_to_u8 of what lte_query would write; no fp32 image is written (hat_lte_query_u8)."""
    lib = _lib.load()
    gh, gw = int(grid[0]), int(grid[1])
    o = out[0] if out.dim() == 4 and out.shape[0] == 1 else out
    if o.dtype != torch.uint8 or not o.is_cuda or tuple(o.shape) != (gh, gw, 3) or o.stride(2) != 1 or o.stride(1) != 3:
        raise RuntimeError(f"lte_query_u8 needs a ({gh},{gw},3) uint8 device destination with interleaved pixels, got {tuple(out.shape)} {out.dtype}")
    args, flops, nbytes = _lte_grid_args("lte_query_u8", pl, coef, freq, inp, H, W, ldc, ldf, grid, cell_yx, out_affine)
    _timed(f"lte_query_kernel<{_TNAME[dtype]}, u8>", flops, lambda: _lib.check(
        lib.hat_lte_query_u8(*args, o.data_ptr(), o.stride(0), int(bool(bgr)), dtype, _stream()), "hat_lte_query_u8"),
        tag=f"lte grid {gh}x{gw} on {H}x{W} -> u8", nbytes=nbytes + 3.0 * gh * gw)


def lte_query_yuv(pl: PackedLte, coef, freq, inp, y, cb, cr, from_rgb, *, H: int, W: int, ldc: int, ldf: int, dtype: int, grid,
                  cell_yx=(0.0, 0.0), out_affine=(1.0, 0.0), sub, depth: int = 8, msb=False):
    """lte_query's grid mode ending in a YCbCr frame: the views Y (1,h,w), Cb, Cr of any subsampling (None, None and sub=None: grey),
    centre-sited = planes_to_yuv of what lte_query would write; no fp32 image is written (hat_lte_query_yuv)."""
    lib = _lib.load()
    gh, gw = int(grid[0]), int(grid[1])
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="lte_query_yuv")
    if tuple(y.shape) != (1, gh, gw):
        raise RuntimeError(f"lte_query_yuv: a {gh}x{gw} grid needs a (1,{gh},{gw}) Y view, got {tuple(y.shape)}")
    args, flops, nbytes = _lte_grid_args("lte_query_yuv", pl, coef, freq, inp, H, W, ldc, ldf, grid, cell_yx, out_affine)
    m, name = _f12(from_rgb), _sub_name(sub, depth)
    _timed(f"lte_query_kernel<{_TNAME[dtype]}, {name}>", flops, lambda: _lib.check(
        lib.hat_lte_query_yuv(*args, C.byref(surf), m, dtype, _stream()), "hat_lte_query_yuv"),
        tag=f"lte grid {gh}x{gw} on {H}x{W} -> {name}", nbytes=nbytes + 3.0 * gh * gw)


LOG2E = 1.4426950408889634


def ocab_attention_log2_supported(C_: int, heads: int, ws: int, wse: int, dtype: int) -> bool:
    """Shapes hat_ocab_attention_log2 (softmax offset in a spare k-slot; q pre-multiplied by log2 e) is built for."""
    return dtype == HAT_BF16 and C_ % heads == 0 and C_ // heads == 24 and ws == 16 and wse == 24 and C_ % 8 == 0


def ocab_attention(q, kv, bias_rot, out, *, B: int, H: int, W: int, C_: int, heads: int, ws: int, wse: int, ldq: int,
                   ldkv: int, ldo: int, dtype: int, q_log2: bool = False):
    """q_log2: q was projected with head_dim^-1/2 * log2(e) folded into its weights (hat_ocab_attention_log2)."""
    lib = _lib.load()
    fn, nm = (lib.hat_ocab_attention_log2, "hat_ocab_attention_log2") if q_log2 else (lib.hat_ocab_attention, "hat_ocab_attention")
    _timed(f"ocab_attn_kernel<{_TNAME[dtype]}>", 2.0 * 2 * wse * wse * C_ * B * H * W, lambda: _lib.check(
        fn(_ptr(q), _ptr(kv), _ptr(bias_rot), _ptr(out), B, H, W, C_, heads, ws, wse, ldq, ldkv, ldo, dtype, _stream()), nm))


# ------------------------------------------------------------------------------------------------
# CAB squeeze conv on the row-sweep kernel (hat_cab_squeeze)
# ------------------------------------------------------------------------------------------------
def cab_squeeze_supported(C_: int, mid: int, W: int, dtype: int) -> bool:
    return dtype == HAT_BF16 and 128 < C_ <= 160 and C_ % 8 == 0 and mid <= 8 and W % 16 == 0


def conv3x3_to_planes_supported(nout: int, cin: int, W: int, dtype: int) -> bool:
    return dtype == HAT_BF16 and cin == 64 and nout <= 8 and W % 16 == 0


def conv3x3_to_planes(x, wpk, bias8, out, *, B: int, H: int, W: int, C_: int, ldx: int, n_out: int, out_scale: float, mean,
                      dtype: int):
    """conv_last on the row-sweep kernel: (conv3x3 + bias) * out_scale + mean -> (B, n_out, H, W) fp32."""
    lib = _lib.load()
    m4 = _mean4(mean)
    _timed("cab_squeeze_kernel<2, planes>", 2.0 * B * H * W * 9 * C_ * n_out, lambda: _lib.check(
        lib.hat_conv3x3_to_planes(_ptr(x), _ptr(wpk), _ptr(bias8), _ptr(out), B, H, W, C_, ldx, n_out, out_scale, m4, dtype,
                                  _stream()), "hat_conv3x3_to_planes"), tag=f"k3 {C_}->{n_out} {H}x{W} row sweep planes")


def conv3x3_to_u8(x, wpk, bias8, out, *, B: int, H: int, W: int, C_: int, ldx: int, h_out: int, w_out: int, out_scale: float, mean,
                  bgr: bool, dtype: int):
    """conv_last with the 8-bit conversion as its epilogue: out (B, h_out, w_out, 3) uint8 = tensor2img of what
    conv3x3_to_planes writes, cropped to the top-left h_out x w_out pixels; no fp32 image is written."""
    lib = _lib.load()
    m4 = _mean4(mean)
    if out.dtype != torch.uint8 or not out.is_cuda or tuple(out.shape) != (B, h_out, w_out, 3) or out.stride(-1) != 1 or out.stride(-2) != 3:
        raise RuntimeError("conv3x3_to_u8 needs a (B,h_out,w_out,3) uint8 device destination with interleaved pixels")
    _timed("cab_squeeze_kernel<2, u8>", 2.0 * B * H * W * 9 * C_ * 3, lambda: _lib.check(
        lib.hat_conv3x3_to_u8(_ptr(x), _ptr(wpk), _ptr(bias8), out.data_ptr(), out.stride(1), out.stride(0), B, H, W, C_, ldx, h_out, w_out,
                              out_scale, m4, int(bgr), dtype, _stream()), "hat_conv3x3_to_u8"), tag=f"k3 {C_}->3 {H}x{W} row sweep u8")


def upfold_supported(cin: int, nout: int, r: int, W: int, dtype: int) -> bool:
    """The folded ending (hat_upfold_*): a 64-channel PixelShuffle(2) stage into a 64 -> 3 conv_last, bf16, W (of the stage's
    input) a multiple of 16."""
    return dtype == HAT_BF16 and cin == 64 and nout == 3 and r == 2 and W >= 16 and W % 16 == 0


def _upfold_flops(B, H, W):
    return 2.0 * B * H * W * 25 * 64 * 12


def _upfold_bytes(B, H, W, out_bytes):
    return float(B * H * W * 64 * 2 + out_bytes)


def upfold_to_planes(x, pf, out, *, B: int, H: int, W: int, ldx: int, out_scale: float, mean, dtype: int):
    """The last PixelShuffle(2) conv and conv_last as one 5x5 conv: x (B,H,W,ldx) bf16 -> (conv_last + bias) * out_scale + mean as
    (B, 3, 2H, 2W) fp32 planes.  pf: packing.PackedUpfold."""
    lib = _lib.load()
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, 3, 2 * H, 2 * W):
        raise RuntimeError(f"upfold_to_planes needs a contiguous (B,3,2H,2W) fp32 device destination, got {tuple(out.shape)} {out.dtype}")
    # through hat_conv's out_mode O_FOLD2_NCHW_F32 (hat_upfold_to_planes behind a HatConvDesc): the form a forward plan records
    d = HatConvDesc()
    d.x, d.w, d.bias, d.out = _ptr(x), _ptr(pf.w), _ptr(pf.bias), _ptr(out)
    d.B, d.H, d.W, d.Cin, d.ldx, d.x_mode = B, H, W, 64, ldx, X_NHWC_T
    d.ksize, d.Kpad, d.nt, d.n_slices, d.n_store = 5, 25 * 64, 1, 1, 12
    d.out_mode, d.act, d.in_scale, d.out_scale, d.dtype = O_FOLD2_NCHW_F32, ACT_NONE, 1.0, out_scale, dtype
    for i in range(3):
        d.mean[i] = float(mean[i])
    _timed("upfold_kernel<planes>", _upfold_flops(B, H, W), lambda: _lib.check(lib.hat_conv(C.byref(d), _stream()), "hat_conv (folded ending)"),
        tag=f"k5 64->2x2x3 {H}x{W} folded planes", nbytes=_upfold_bytes(B, H, W, B * 12 * H * W * 4))


def upfold_to_u8(x, pf, out, *, B: int, H: int, W: int, ldx: int, h_out: int, w_out: int, out_scale: float, mean, bgr: bool, dtype: int):
    """The folded ending with the 8-bit conversion as its epilogue: out (B, h_out, w_out, 3) uint8 = planes_to_u8 of what
    upfold_to_planes writes, cropped to the top-left h_out x w_out pixels; no fp32 image is written."""
    lib = _lib.load()
    if out.dtype != torch.uint8 or not out.is_cuda or tuple(out.shape) != (B, h_out, w_out, 3) or out.stride(-1) != 1 or out.stride(-2) != 3:
        raise RuntimeError("upfold_to_u8 needs a (B,h_out,w_out,3) uint8 device destination with interleaved pixels")
    _timed("upfold_kernel<u8>", _upfold_flops(B, H, W), lambda: _lib.check(
        lib.hat_upfold_to_u8(_ptr(x), _ptr(pf.w), _ptr(pf.bias), out.data_ptr(), out.stride(1), out.stride(0), B, H, W, ldx, h_out, w_out,
                             out_scale, float(mean[0]), float(mean[1]), float(mean[2]), int(bgr), dtype, _stream()), "hat_upfold_to_u8"),
        tag=f"k5 64->2x2x3 {H}x{W} folded u8", nbytes=_upfold_bytes(B, H, W, B * h_out * w_out * 3))


def u8_to_planes(src, dst, *, bgr: bool = False):
    """src (B, h, w, 3) uint8 (rows may be pitched: stride(-3) >= 3 w) -> dst (B, 3, Hp, Wp) fp32 = float(src) / 255 as
    planes, the rows and columns past (h, w) filled by reflection (hat_u8_to_planes)."""
    lib = _lib.load()
    B, h, w, c = src.shape
    if c != 3 or src.dtype != torch.uint8 or src.stride(-1) != 1 or src.stride(-2) != 3 or dst.dtype != torch.float32:
        raise RuntimeError("u8_to_planes needs (B,h,w,3) uint8 with interleaved pixels and an fp32 destination")
    if not src.is_cuda:
        raise RuntimeError("HAT HIP ops need device tensors (no CPU path exists)")
    if dst.dim() != 4 or dst.shape[0] != B or dst.shape[1] != 3 or dst.shape[2] < h or dst.shape[3] < w or dst.device != src.device:
        raise RuntimeError(f"u8_to_planes needs a (B,3,Hp>=h,Wp>=w) destination on {src.device}, got {tuple(dst.shape)} on {dst.device} "
                           f"for frames {tuple(src.shape)}")
    _timed("u8_to_planes_kernel", 0.0, lambda: _lib.check(
        lib.hat_u8_to_planes(src.data_ptr(), src.stride(1), src.stride(0), _ptr(dst), B, h, w, dst.shape[2], dst.shape[3], int(bgr),
                             _stream()), "hat_u8_to_planes"), tag=f"u8 {h}x{w} -> planes {dst.shape[2]}x{dst.shape[3]}")


def planes_to_u8(src, dst, *, bgr: bool = False):
    """src (B, 3, Hs, Ws) fp32 planes -> dst (B, h_out, w_out, 3) uint8 (rows may be pitched), the top-left crop, converted as
    the reference's tensor2img converts: clamp to [0, 1], x255 in fp32, round half to even (hat_planes_to_u8)."""
    lib = _lib.load()
    B, c, Hs, Ws = src.shape
    if c != 3 or src.dtype != torch.float32 or dst.dtype != torch.uint8 or dst.shape[0] != B or dst.shape[3] != 3 or dst.stride(-1) != 1 \
            or dst.stride(-2) != 3 or not dst.is_cuda:
        raise RuntimeError("planes_to_u8 needs (B,3,Hs,Ws) fp32 planes and a (B,h,w,3) uint8 device destination with interleaved pixels")
    _timed("planes_to_u8_kernel", 0.0, lambda: _lib.check(
        lib.hat_planes_to_u8(_ptr(src), B, Hs, Ws, dst.data_ptr(), dst.stride(1), dst.stride(0), dst.shape[1], dst.shape[2], int(bgr),
                             _stream()), "hat_planes_to_u8"), tag=f"planes {Hs}x{Ws} -> u8 {dst.shape[1]}x{dst.shape[2]}")


ENSEMBLE_SIZES = (1, 2, 4, 8)   # members of the geometric self-ensemble: the first n of the eight (HATEngine.forward_ensemble)


def ensemble_members(n) -> int:
    """The member count a caller asked for: 1, 2, 4 or 8 as an int (a bool is not a count); anything else is a ValueError."""
    if isinstance(n, bool) or not isinstance(n, int) or n not in ENSEMBLE_SIZES:
        raise ValueError(f"the self-ensemble runs the first 1, 2, 4 or 8 of the eight flips / transposes, got {n!r}")
    return n


def dihedral(src, dst, *, op: int, inverse: bool = False, alpha: float = 1.0, accumulate: bool = False):
    """src (..., H, W) fp32 -> dst (..., H', W') fp32, the leading axes are planes: dst[T(y, x)] = (accumulate ? dst : 0) + alpha *
    src[y, x] with T member `op` = v | h << 1 | t << 2 of the eight flips / transposes (v: reverse W, h: reverse H, t: swap H and W,
    in that order) or, with inverse, its inverse; (H', W') = (W, H) when op contains t (hat_dihedral_f32)."""
    lib = _lib.load()
    if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.dim() < 2 or src.device != dst.device:
        raise RuntimeError(f"dihedral needs fp32 planes on one device, got {src.dtype} on {src.device} and {dst.dtype} on {dst.device}")
    if not 0 <= int(op) <= 7:
        raise RuntimeError(f"dihedral: op is one of the eight members 0..7, got {op}")
    H, W = src.shape[-2:]
    want = tuple(src.shape[:-2]) + ((W, H) if op & 4 else (H, W))
    if tuple(dst.shape) != want:
        raise RuntimeError(f"dihedral: member {op} of {tuple(src.shape)} planes needs a {want} destination, got {tuple(dst.shape)}")
    planes = src.numel() // (H * W)
    _timed("dihedral_transpose_kernel" if op & 4 else "dihedral_flip_kernel", 0.0, lambda: _lib.check(
        lib.hat_dihedral_f32(_ptr(src), _ptr(dst), planes, H, W, int(op), int(bool(inverse)), float(alpha), int(bool(accumulate)), _stream()),
        "hat_dihedral_f32"), tag=f"dihedral op {op}{' inv' if inverse else ''} {planes}x{H}x{W}", nbytes=4.0 * src.numel() * (3 if accumulate else 2))


# ---- MATLAB bicubic imresize (definition: resize.py; kernels: csrc/hat_resize.hip) ----
resize_calls = 0            # imresize calls = hat_imresize_rows + hat_imresize_cols_* pairs
_RESIZE_TABLES_KEPT = 32    # axes; a folder of images of many sizes must not pile tables up
_resize_tables = collections.OrderedDict()   # (device, in_len, out_len, scale, antialiasing) -> the axis' uploaded tables, least recent first
_resize_mid = {}            # (device, stream) -> ONE flat fp32 buffer, the general route's intermediate: it only grows


def _resize_workspace(dev, B: int, oh: int, w: int):
    """The (B,3,oh,w) fp32 intermediate as a view of the device's and stream's one grow-only buffer: launches on one stream are
    ordered, so they may share it; another stream gets its own.  A buffer that is outgrown goes back to torch's allocator, which
    hands it out again in stream order."""
    key, n = (str(dev), _stream()), B * 3 * oh * w
    buf = _resize_mid.get(key)
    if buf is None or buf.numel() < n:
        _resize_mid.pop(key, None)
        buf = _resize_mid[key] = torch.empty(n, dtype=torch.float32, device=dev)
    return buf[:n].view(B, 3, oh, w)


def _resize_axis(dev, in_len: int, scale: float, antialiasing: bool) -> dict:
    """One axis' tables on `dev`, built on the host by resize.tables and cached: w, src (device tensors), P, out."""
    import numpy as np

    from . import resize as _rz
    out_len = _rz.out_length(in_len, scale)
    key = (str(dev), int(in_len), out_len, float(scale), bool(antialiasing))
    t = _resize_tables.get(key)
    if t is not None:
        _resize_tables.move_to_end(key)
    else:
        try:
            w, s, _, _ = _rz.tables(in_len, out_len, scale, antialiasing)
        except ValueError as e:
            raise RuntimeError(str(e)) from e
        t = {"w": torch.from_numpy(w).to(dev).contiguous(), "src": torch.from_numpy(_rz.mirror(s, in_len).astype(np.int32)).to(dev).contiguous(),
             "P": w.shape[1], "out": out_len}
        _resize_tables[key] = t
        while len(_resize_tables) > _RESIZE_TABLES_KEPT:
            _resize_tables.popitem(last=False)
    return t


def imresize(src, scale: float, *, antialiasing: bool = True, dst=None, to: str = "planes", pad_to=None, bgr: bool = False):
    """resize.imresize on the device, bit for bit.  src: (B,h,w,3) uint8 frames (rows may be pitched; value float(v) / 255) or
    (B,3,h,w) fp32 planes.  to='planes': -> (B,3,Hp,Wp) fp32, (Hp, Wp) = pad_to (default: the resized size), the rows and
    columns past the resized image filled by reflection as hat_u8_to_planes fills them; to='u8': -> (B,oh,ow,3) uint8 by
    tensor2img's conversion.  bgr: the bytes of a uint8 side are B, G, R.  dst: the caller's destination (default: a fresh
    one; with it a second call of the same shape allocates nothing: the last 32 axes' tables are kept, and the intermediate is one
    grow-only buffer per device and stream).  Two launches, any scale, either direction."""
    global resize_calls
    lib = _lib.load()
    if to not in ("planes", "u8"):
        raise RuntimeError(f"imresize: to is 'planes' or 'u8', got {to!r}")
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dim() != 4:
        raise RuntimeError("imresize needs a (B,h,w,3) uint8 or (B,3,h,w) fp32 device tensor (no CPU path exists: resize.imresize is the host definition)")
    u8 = src.dtype == torch.uint8
    if u8:
        B, h, w, c = src.shape
        if c != 3 or src.stride(3) != 1 or src.stride(2) != 3:
            raise RuntimeError(f"imresize needs (B,h,w,3) uint8 frames with interleaved pixels, got {tuple(src.shape)}")
    else:
        B, c, h, w = src.shape
        if c != 3 or src.dtype != torch.float32 or not src.is_contiguous():
            raise RuntimeError(f"imresize needs contiguous (B,3,h,w) fp32 planes, got {tuple(src.shape)} {src.dtype}")
    dev = src.device
    th, tw = _resize_axis(dev, h, scale, antialiasing), _resize_axis(dev, w, scale, antialiasing)
    oh, ow = th["out"], tw["out"]
    if to == "planes":
        Hp, Wp = (oh, ow) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
        if Hp < oh or Wp < ow or Hp - oh >= oh or Wp - ow >= ow:
            raise RuntimeError(f"a {oh}x{ow} image cannot be reflect-padded to {Hp}x{Wp}: the padding must be smaller than the image")
        shape, dtype = (B, 3, Hp, Wp), torch.float32
    else:
        if pad_to is not None:
            raise RuntimeError("imresize: pad_to goes with to='planes'")
        shape, dtype = (B, oh, ow, 3), torch.uint8
    if dst is None:
        dst = torch.empty(shape, dtype=dtype, device=dev)
    elif tuple(dst.shape) != shape or dst.dtype != dtype or dst.device != dev or (to == "planes" and not dst.is_contiguous()) \
            or (to == "u8" and (dst.stride(3) != 1 or dst.stride(2) != 3)):
        raise RuntimeError(f"imresize: dst must be a {shape} {dtype} tensor on {dev}, got {tuple(dst.shape)} {dst.dtype} on {dst.device}")
    mid = _resize_workspace(dev, B, oh, w)
    _timed(f"resize_rows_kernel<{'u8' if u8 else 'f32'}>", 2.0 * B * 3 * oh * w * th["P"], lambda: _lib.check(
        lib.hat_imresize_rows(src.data_ptr(), int(u8), src.stride(1) if u8 else 0, src.stride(0) if u8 else 0, int(bgr and u8), _ptr(mid),
                              B, h, w, oh, _ptr(th["w"]), _ptr(th["src"]), th["P"], th["w"].numel(), _stream()), "hat_imresize_rows"),
        tag=f"imresize rows {h}x{w} -> {oh}x{w}", nbytes=B * 3.0 * (h * w * (1 if u8 else 4) + 4.0 * oh * w))
    if to == "planes":
        _timed("resize_cols_kernel<planes>", 2.0 * B * 3 * Hp * Wp * tw["P"], lambda: _lib.check(
            lib.hat_imresize_cols_to_planes(_ptr(mid), B, oh, w, ow, _ptr(tw["w"]), _ptr(tw["src"]), tw["P"], tw["w"].numel(), _ptr(dst),
                                            Hp, Wp, _stream()), "hat_imresize_cols_to_planes"),
            tag=f"imresize cols {oh}x{w} -> planes {Hp}x{Wp}", nbytes=B * 3.0 * 4.0 * (oh * w + Hp * Wp))
    else:
        _timed("resize_cols_kernel<u8>", 2.0 * B * 3 * oh * ow * tw["P"], lambda: _lib.check(
            lib.hat_imresize_cols_to_u8(_ptr(mid), B, oh, w, ow, _ptr(tw["w"]), _ptr(tw["src"]), tw["P"], tw["w"].numel(), dst.data_ptr(),
                                        dst.stride(1), dst.stride(0), int(bgr), _stream()), "hat_imresize_cols_to_u8"),
            tag=f"imresize cols {oh}x{w} -> u8 {oh}x{ow}", nbytes=B * 3.0 * (4.0 * oh * w + oh * ow))
    resize_calls += 1
    return dst


# ---- Pillow's 8-bit bicubic resize and the ESC-LTE benchmark's PSNR (definitions: resize.pil_bicubic_u8, metrics.arb_psnr; kernels:
# csrc/hat_pil_resize.hip) ----
_pil_mid = {}               # (device, stream) -> ONE flat uint8 buffer, the image between the two passes: it only grows
_arb_psnr_ws = {}           # (device, stream) -> (the partials' workspace, the (2,) float64 result)


def _pil_axis(dev, in_len: int, out_len: int) -> dict:
    """One axis' Pillow tables on `dev` (resize.pil_tables), cached beside the MATLAB ones: coef, bounds (device tensors), K."""
    from . import resize as _rz
    key = (str(dev), "pil", int(in_len), int(out_len))
    t = _resize_tables.get(key)
    if t is not None:
        _resize_tables.move_to_end(key)
    else:
        coef, bounds = _rz.pil_tables(in_len, out_len)
        t = {"coef": torch.from_numpy(coef).to(dev).contiguous(), "bounds": torch.from_numpy(bounds).to(dev).contiguous(), "K": coef.shape[1]}
        _resize_tables[key] = t
        while len(_resize_tables) > _RESIZE_TABLES_KEPT:
            _resize_tables.popitem(last=False)
    return t


def pil_resize_u8(src, size, *, dst=None):
    """resize.pil_bicubic_u8 on the device, bit for bit: src (h,w,3) uint8 (rows may be pitched) -> (size[0], size[1], 3) uint8,
    PIL.Image.resize's 8-bit bicubic (hat_pil_resize_u8: the horizontal pass into a uint8 intermediate, then the vertical pass).
    dst: the caller's destination (rows may be pitched; bytes past a row's width stay as they are); default: a fresh tensor."""
    lib = _lib.load()
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or src.stride(2) != 1 \
            or src.stride(1) != 3:
        raise RuntimeError(f"pil_resize_u8 needs an (h,w,3) uint8 frame with interleaved pixels, got {tuple(getattr(src, 'shape', ()))} "
                           f"{getattr(src, 'dtype', type(src).__name__)}")
    if not src.is_cuda:
        raise RuntimeError("HAT HIP ops need device tensors (no CPU path exists: resize.pil_bicubic_u8 is the host definition)")
    h, w = int(src.shape[0]), int(src.shape[1])
    oh, ow = int(size[0]), int(size[1])
    if min(h, w, oh, ow) < 1:
        raise RuntimeError(f"pil_resize_u8: a resize of {h}x{w} to {oh}x{ow} has an empty side")
    dev = src.device
    if dst is None:
        dst = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
    elif not isinstance(dst, torch.Tensor) or tuple(dst.shape) != (oh, ow, 3) or dst.dtype != torch.uint8 or dst.device != dev \
            or dst.stride(2) != 1 or dst.stride(1) != 3:
        raise RuntimeError(f"pil_resize_u8: dst must be a {(oh, ow, 3)} uint8 tensor on {dev} with interleaved pixels, got "
                           f"{tuple(getattr(dst, 'shape', ()))} {getattr(dst, 'dtype', type(dst).__name__)}")
    tw, th = _pil_axis(dev, w, ow), _pil_axis(dev, h, oh)
    key, n = (str(dev), _stream()), 3 * ow * h
    mid = _pil_mid.get(key)
    if mid is None or mid.numel() < n:
        _pil_mid.pop(key, None)
        mid = _pil_mid[key] = torch.empty(n, dtype=torch.uint8, device=dev)
    src_pitch = src.stride(0) if h > 1 else 3 * w
    dst_pitch = dst.stride(0) if oh > 1 else 3 * ow
    _timed("pil_resize_h_kernel+pil_resize_v_kernel", 2.0 * 3 * ow * (h * tw["K"] + oh * th["K"]), lambda: _lib.check(
        lib.hat_pil_resize_u8(src.data_ptr(), src_pitch, h, w, _ptr(mid), dst.data_ptr(), dst_pitch, oh, ow, _ptr(tw["coef"]),
                              _ptr(tw["bounds"]), tw["K"], _ptr(th["coef"]), _ptr(th["bounds"]), th["K"], _stream()), "hat_pil_resize_u8"),
        tag=f"pil bicubic {h}x{w} -> {oh}x{ow}", nbytes=3.0 * (h * w + 2 * h * ow + oh * ow))
    return dst


ARB_PSNR_MODES = (None, "benchmark", "div2k")   # utils.py:132-149: no eval_type, the weighted channel sum, all of RGB


def arb_psnr_workspace_bytes(h: int, w: int, shave: int) -> int:
    """Bytes of workspace hat_arb_psnr needs for an (h,w) ground truth; raises for what it refuses (a pure host query)."""
    lib = _lib.load()
    n = C.c_int64(0)
    _lib.check(lib.hat_arb_psnr_workspace_bytes(int(h), int(w), int(shave), C.byref(n)), "hat_arb_psnr_workspace_bytes")
    return n.value


def arb_psnr(pred, gt, *, mode, shave: int, sums=None):
    """metrics.arb_psnr's sum on the device: pred (3,ph,pw) or (1,3,ph,pw) contiguous fp32 planes, gt (h,w,3) uint8 (rows may be
    pitched), h <= ph, w <= pw: the top-left (h, w) of pred is scored.  mode: None | 'benchmark' | 'div2k' (ARB_PSNR_MODES); shave
    pixels off every side.  -> sums, a (2,) float64 device tensor (the caller's, or the device's and stream's own): the sum of
    squares and the number of terms (hat_arb_psnr).  The same inputs give the same bits."""
    lib = _lib.load()
    if mode not in ARB_PSNR_MODES:
        raise RuntimeError(f"arb_psnr: mode is one of {ARB_PSNR_MODES}, got {mode!r}")
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.float32 or not pred.is_contiguous() \
            or tuple(pred.shape[:-2]) not in ((3,), (1, 3)):
        raise RuntimeError(f"arb_psnr needs contiguous (3,h,w) fp32 planes, got {tuple(getattr(pred, 'shape', ()))} "
                           f"{getattr(pred, 'dtype', type(pred).__name__)}")
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or gt.dim() != 3 or gt.shape[2] != 3 or gt.stride(2) != 1 or gt.stride(1) != 3:
        raise RuntimeError(f"arb_psnr needs an (h,w,3) uint8 ground truth with interleaved pixels, got {tuple(getattr(gt, 'shape', ()))}")
    if not pred.is_cuda or gt.device != pred.device:
        raise RuntimeError("HAT HIP ops need device tensors on one device (no CPU path exists: metrics.arb_psnr is the host definition)")
    ph, pw = int(pred.shape[-2]), int(pred.shape[-1])
    h, w = int(gt.shape[0]), int(gt.shape[1])
    dev = pred.device
    need = arb_psnr_workspace_bytes(h, w, shave)
    key = (str(dev), _stream())
    ws = _arb_psnr_ws.get(key)
    if ws is None or ws[0].numel() < need:
        ws = _arb_psnr_ws[key] = (torch.empty(max(need, 8192), dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.float64, device=dev))
    if sums is None:
        sums = ws[1]
    elif sums.dtype != torch.float64 or tuple(sums.shape) != (2,) or sums.device != dev:
        raise RuntimeError(f"arb_psnr: sums must be a (2,) float64 tensor on {dev}")
    _timed("arb_psnr_kernel", 0.0, lambda: _lib.check(
        lib.hat_arb_psnr(_ptr(pred), ph, pw, gt.data_ptr(), gt.stride(0) if h > 1 else 3 * w, h, w, int(mode == "benchmark"), int(shave),
                         _ptr(sums), _ptr(ws[0]), _stream()), "hat_arb_psnr"),
        tag=f"arb psnr {h}x{w} shave {shave} {mode}", nbytes=15.0 * (h - 2 * shave) * (w - 2 * shave))
    return sums


def yuv420_views(frame, fmt: str = "nv12"):
    """yuv_views for the three 4:2:0 layouts of yuv.FORMATS: frame (B, 3h/2, w) -> views y (B,h,w), cb, cr (B,h/2,w/2), the torch
    twin of yuv.split.  The chroma views step 2 samples for nv12 / nv21 and 1 for i420."""
    from . import yuv as _yuv
    return yuv_views(frame, _yuv.check_fmt(fmt))


def _yuv_block(y, cb, cr, what: str):
    """The C frame block (y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride) of three uint8 device views, or of three
    uint16 ones (deep samples): pitches, strides and the step are in BYTES either way."""
    if y.dim() != 3 or y.dtype not in (torch.uint8, torch.uint16) or cb.dtype != y.dtype or cr.dtype != y.dtype:
        raise TypeError(f"{what} needs uint8 (or uint16) (B,h,w) / (B,h/2,w/2) views, got {y.dtype} {tuple(y.shape)}")
    if not (y.is_cuda and cb.is_cuda and cr.is_cuda):
        raise RuntimeError("HAT HIP ops need device tensors (no CPU path exists)")
    B, h, w = y.shape
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise RuntimeError(f"{what}: 4:2:0 frames need even sizes, got {h}x{w}")
    if tuple(cb.shape) != (B, h // 2, w // 2) or tuple(cr.shape) != tuple(cb.shape) or cb.stride() != cr.stride() or y.stride(2) != 1 \
            or cb.stride(2) not in (1, 2):
        raise RuntimeError(f"{what} needs Y (B,h,w) with unit step and Cb, Cr (B,h/2,w/2) of one pitch with a step of 1 or 2 samples")
    n = y.element_size()
    return [y.data_ptr(), n * y.stride(1), n * y.stride(0), cb.data_ptr(), cr.data_ptr(), n * cb.stride(1), n * cb.stride(2), n * cb.stride(0)]


def _deep_args(y, depth, msb, what: str):
    """() for byte views, (depth, msb) for uint16 views: the width must agree with the dtype."""
    if y.dtype == torch.uint8:
        if depth not in (None, 8):
            raise TypeError(f"{what}: uint8 views hold 8-bit samples, not depth {depth}")
        return ()
    if depth not in (10, 12, 16):
        raise TypeError(f"{what}: uint16 views need depth 10, 12 or 16 (uint8 views hold 8-bit samples), got {depth}")
    return (int(depth), int(bool(msb)))


def _deep_entry(entry: str, deep):
    """(C entry point, record-name suffix, tag suffix) of the 8-bit (deep == ()) or the deep-sample twin of a 4:2:0 launch."""
    return (entry.format("p16"), "<u16>", f"p{deep[0]}") if deep else (entry.format(""), "", "")


def _planes_dst(what: str, dst, y, contiguous: bool = False):
    """dst holds the padded fp32 RGB planes of the frames whose Y view is y (B,h,w)."""
    B, h, w = y.shape
    if dst.dtype != torch.float32 or dst.dim() != 4 or dst.shape[0] != B or dst.shape[1] != 3 or dst.shape[2] < h or dst.shape[3] < w \
            or dst.device != y.device or (contiguous and not dst.is_contiguous()):
        raise RuntimeError(f"{what} needs a {'contiguous ' if contiguous else ''}(B,3,Hp>=h,Wp>=w) fp32 destination on {y.device}, got "
                           f"{tuple(dst.shape)} {dst.dtype} on {dst.device} for frames {tuple(y.shape)}")


def _planes_src(what: str, src, y, contiguous: bool = False):
    """src holds fp32 RGB planes for the frames whose Y view is y (the kernel's own checks see that they are large enough)."""
    if src.dim() != 4 or src.shape[0] != y.shape[0] or src.shape[1] != 3 or src.dtype != torch.float32 or src.device != y.device \
            or (contiguous and not src.is_contiguous()):
        raise RuntimeError(f"{what} needs {'contiguous ' if contiguous else ''}(B,3,Hs,Ws) fp32 planes on {y.device}, got {tuple(src.shape)} "
                           f"{src.dtype} on {src.device}")


def _f12(m):
    m = [float(v) for v in m]
    if len(m) != 12:
        raise RuntimeError("a colour matrix is 12 floats (yuv.csc)")
    return (C.c_float * 12)(*m)


def yuv420_to_planes(y, cb, cr, dst, to_rgb, *, depth=None, msb=False):
    """Y (B,h,w), Cb, Cr (B,h/2,w/2) uint8 views (yuv420_views; rows may be pitched) -> dst (B,3,Hp,Wp) fp32 RGB planes, rows and
    columns past (h, w) filled by reflection; the conversion is yuv.yuv420_to_planes' (hat_yuv420_to_planes).  uint16 views with
    depth 10 / 12 / 16 and msb (MSB-aligned words): hat_yuv420p16_to_planes."""
    lib = _lib.load()
    blk = _yuv_block(y, cb, cr, "yuv420_to_planes")
    deep = _deep_args(y, depth, msb, "yuv420_to_planes")
    B, h, w = y.shape
    _planes_dst("yuv420_to_planes", dst, y)
    m = _f12(to_rgb)
    entry, u16, p = _deep_entry("hat_yuv420{}_to_planes", deep)
    _timed("yuv420_to_planes_kernel" + u16, 0.0, lambda: _lib.check(
        getattr(lib, entry)(*blk, _ptr(dst), B, h, w, dst.shape[2], dst.shape[3], m, *deep, _stream()), entry),
        tag=f"yuv420{p} {h}x{w} -> planes {dst.shape[2]}x{dst.shape[3]}")


def planes_to_yuv420(src, y, cb, cr, from_rgb, *, depth=None, msb=False):
    """src (B,3,Hs,Ws) fp32 planes -> the top-left h x w pixels as Y (B,h,w), Cb, Cr (B,h/2,w/2) uint8 views, converted as
    yuv.planes_to_yuv420 converts (hat_planes_to_yuv420).  uint16 views with depth / msb: hat_planes_to_yuv420p16."""
    lib = _lib.load()
    blk = _yuv_block(y, cb, cr, "planes_to_yuv420")
    deep = _deep_args(y, depth, msb, "planes_to_yuv420")
    B, h, w = y.shape
    _planes_src("planes_to_yuv420", src, y)
    m = _f12(from_rgb)
    entry, u16, p = _deep_entry("hat_planes_to_yuv420{}", deep)
    _timed("planes_to_yuv420_kernel" + u16, 0.0, lambda: _lib.check(
        getattr(lib, entry)(_ptr(src), B, src.shape[2], src.shape[3], *blk, h, w, m, *deep, _stream()), entry),
        tag=f"planes {src.shape[2]}x{src.shape[3]} -> yuv420{p} {h}x{w}")


def conv3x3_to_yuv420(x, wpk, bias8, y, cb, cr, *, B: int, H: int, W: int, C_: int, ldx: int, out_scale: float, mean, from_rgb, dtype: int,
                      depth=None, msb=False):
    """conv_last with the 4:2:0 conversion as its epilogue: Y (B,h,w), Cb, Cr (B,h/2,w/2) = planes_to_yuv420 of what
    conv3x3_to_planes writes, cropped to the top-left h x w pixels; neither an fp32 nor an RGB byte image is written.
    uint16 views with depth / msb: hat_conv3x3_to_yuv420p16."""
    lib = _lib.load()
    blk = _yuv_block(y, cb, cr, "conv3x3_to_yuv420")
    deep = _deep_args(y, depth, msb, "conv3x3_to_yuv420")
    if y.shape[0] != B:
        raise RuntimeError(f"conv3x3_to_yuv420: destination batch {y.shape[0]} != {B}")
    m4 = _mean4(mean)
    m = _f12(from_rgb)
    entry, _, p = _deep_entry("hat_conv3x3_to_yuv420{}", deep)
    _timed(f"cab_squeeze_kernel<2, yuv420{'p16' if deep else ''}>", 2.0 * B * H * W * 9 * C_ * 3, lambda: _lib.check(
        getattr(lib, entry)(_ptr(x), _ptr(wpk), _ptr(bias8), *blk, B, H, W, C_, ldx, y.shape[1], y.shape[2], out_scale, m4, m, dtype,
                            *deep, _stream()), entry), tag=f"k3 {C_}->3 {H}x{W} row sweep yuv420{p}")


def yuv_views(frame, fmt: str):
    """frame (B, rows, w) uint8 (uint16: deep samples) in the standard layout of any `fmt` of yuv.LAYOUTS (rows w samples apart) ->
    views y (B,h,w), cb, cr (B, h >> sub_y, w >> sub_x): the torch twin of yuv.split_fmt; cb = cr = None for 'gray'."""
    from . import yuv as _yuv
    sub_x, sub_y, kind = _yuv.check_layout(fmt)
    if frame.dim() != 3 or frame.dtype not in (torch.uint8, torch.uint16) or frame.stride(2) != 1 or frame.stride(1) != frame.shape[2]:
        raise RuntimeError(f"expected (B,rows,w) uint8 frames with packed rows, got {tuple(frame.shape)} {frame.dtype} strides {frame.stride()}")
    h, w = _yuv.frame_size_fmt(frame.shape, fmt)
    if kind == "gray":
        return frame, None, None
    B, ch, cw, off = frame.shape[0], h >> sub_y, w >> sub_x, frame.storage_offset() + h * w
    if kind == "planar":
        st, o_cb, o_cr = (frame.stride(0), cw, 1), off, off + ch * cw
    else:
        st, o_cb, o_cr = (frame.stride(0), 2 * cw, 2), off + (kind == "semi_vu"), off + (kind == "semi")
    return frame[:, :h], frame.as_strided((B, ch, cw), st, o_cb), frame.as_strided((B, ch, cw), st, o_cr)


def yuv_surface(y, cb, cr, *, sub, depth: int = 8, msb=False, what: str = "yuv_surface"):
    """The HatYuvSurface of three device views (cb = cr = None and sub = None: grey): pitches, strides and the step in BYTES;
    sub = (sub_x, sub_y).  The struct holds raw pointers: keep the views alive while it is used."""
    if y.dim() != 3 or y.dtype not in (torch.uint8, torch.uint16):
        raise TypeError(f"{what} needs uint8 (or uint16) (B,h,w) views, got {y.dtype} {tuple(y.shape)}")
    if (y.dtype == torch.uint8) != (depth == 8) or depth not in (8, 10, 12, 16):
        raise TypeError(f"{what}: depth {depth} does not go with {y.dtype} views (uint8 holds 8-bit samples, uint16 10, 12 or 16 bits)")
    if (cb is None) != (cr is None) or (cb is None) != (sub is None):
        raise RuntimeError(f"{what}: a grey surface has neither Cb nor Cr nor a subsampling; every other one has all three")
    if not y.is_cuda or y.stride(2) != 1:
        raise RuntimeError("HAT HIP ops need device tensors with unit-step rows (no CPU path exists)")
    n, (B, h, w) = y.element_size(), y.shape
    s = _lib.HatYuvSurface(y=y.data_ptr(), y_pitch=n * y.stride(1), y_bstride=n * y.stride(0), depth=int(depth), msb=int(bool(msb)))
    if cb is not None:
        sx, sy = int(sub[0]), int(sub[1])
        if (sx, sy) not in ((1, 1), (1, 0), (0, 0)) or (sx and w % 2) or (sy and h % 2):
            raise RuntimeError(f"{what}: a {h}x{w} frame has no chroma subsampling {(sx, sy)} (w even where sub_x = 1, h where sub_y = 1)")
        if cb.dtype != y.dtype or cr.dtype != y.dtype or not (cb.is_cuda and cr.is_cuda) or tuple(cb.shape) != (B, h >> sy, w >> sx) \
                or tuple(cr.shape) != tuple(cb.shape) or cb.stride() != cr.stride() or cb.stride(2) not in (1, 2):
            raise RuntimeError(f"{what} needs Cb, Cr ({B},{h >> sy},{w >> sx}) views of Y's dtype and one pitch with a step of 1 or 2 samples")
        s.cb, s.cr, s.c_pitch, s.c_step, s.c_bstride, s.sub_x, s.sub_y = cb.data_ptr(), cr.data_ptr(), n * cb.stride(1), n * cb.stride(2), \
            n * cb.stride(0), sx, sy
    return s


def _sub_name(sub, depth):
    return ("gray" if sub is None else {(1, 1): "yuv420", (1, 0): "yuv422", (0, 0): "yuv444"}[tuple(sub)]) + ("" if depth == 8 else f"p{depth}")


def _siting(sub, siting):
    """The siting the layout makes of `siting` (yuv.effective_siting: 'center' on 4:4:4 and grey, 'left' for 'topleft' on 4:2:2)
    and its C code; an unknown siting is refused naming yuv.SITINGS."""
    from . import yuv as _yuv
    eff = _yuv.effective_siting(sub, siting)
    return eff, _yuv.SITINGS.index(eff)


def yuv_to_planes(y, cb, cr, dst, to_rgb, *, sub, depth: int = 8, msb=False, siting: str = "center"):
    """Y (B,h,w), Cb, Cr (B, h >> sub_y, w >> sub_x) views (yuv_views; None, None and sub=None: grey) -> dst (B,3,Hp,Wp) fp32 RGB
    planes, rows and columns past (h, w) filled by reflection: yuv.yuv_to_planes' conversion (hat_yuv_to_planes; with a siting
    that leaves an axis co-sited, hat_yuv_to_planes_sited)."""
    lib = _lib.load()
    eff, code = _siting(sub, siting)
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="yuv_to_planes")
    B, h, w = y.shape
    _planes_dst("yuv_to_planes", dst, y, contiguous=True)
    m, name = _f12(to_rgb), _sub_name(sub, depth)
    if code:
        _timed(f"yuv_to_planes_sited_kernel<{name}, {eff}>", 0.0, lambda: _lib.check(
            lib.hat_yuv_to_planes_sited(C.byref(surf), code, _ptr(dst), B, h, w, dst.shape[2], dst.shape[3], m, _stream()),
            "hat_yuv_to_planes_sited"), tag=f"{name} {eff} {h}x{w} -> planes {dst.shape[2]}x{dst.shape[3]}")
        return
    _timed(f"yuv_to_planes_kernel<{name}>", 0.0, lambda: _lib.check(
        lib.hat_yuv_to_planes(C.byref(surf), _ptr(dst), B, h, w, dst.shape[2], dst.shape[3], m, _stream()), "hat_yuv_to_planes"),
        tag=f"{name} {h}x{w} -> planes {dst.shape[2]}x{dst.shape[3]}")


def planes_to_yuv(src, y, cb, cr, from_rgb, *, sub, depth: int = 8, msb=False, siting: str = "center"):
    """src (B,3,Hs,Ws) fp32 planes -> the top-left h x w pixels as Y (B,h,w), Cb, Cr views of any subsampling (or grey), converted
    as yuv.planes_to_yuv converts (hat_planes_to_yuv; with a siting that leaves an axis co-sited, hat_planes_to_yuv_sited)."""
    lib = _lib.load()
    eff, code = _siting(sub, siting)
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="planes_to_yuv")
    B, h, w = y.shape
    _planes_src("planes_to_yuv", src, y, contiguous=True)
    m, name = _f12(from_rgb), _sub_name(sub, depth)
    if code:
        _timed(f"planes_to_yuv_sited_kernel<{name}, {eff}>", 0.0, lambda: _lib.check(
            lib.hat_planes_to_yuv_sited(_ptr(src), B, src.shape[2], src.shape[3], C.byref(surf), code, h, w, m, _stream()),
            "hat_planes_to_yuv_sited"), tag=f"planes {src.shape[2]}x{src.shape[3]} -> {name} {eff} {h}x{w}")
        return
    _timed(f"planes_to_yuv_kernel<{name}>", 0.0, lambda: _lib.check(
        lib.hat_planes_to_yuv(_ptr(src), B, src.shape[2], src.shape[3], C.byref(surf), h, w, m, _stream()), "hat_planes_to_yuv"),
        tag=f"planes {src.shape[2]}x{src.shape[3]} -> {name} {h}x{w}")


def conv3x3_to_yuv(x, wpk, bias8, y, cb, cr, *, sub, B: int, H: int, W: int, C_: int, ldx: int, out_scale: float, mean, from_rgb, dtype: int,
                   depth: int = 8, msb=False):
    """conv_last with the YCbCr conversion of any subsampling (or grey) as its epilogue: planes_to_yuv of what conv3x3_to_planes
    writes, cropped to the top-left h x w pixels of the views; no fp32 image is written (hat_conv3x3_to_yuv)."""
    lib = _lib.load()
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="conv3x3_to_yuv")
    if y.shape[0] != B:
        raise RuntimeError(f"conv3x3_to_yuv: destination batch {y.shape[0]} != {B}")
    m4, m, name = _mean4(mean), _f12(from_rgb), _sub_name(sub, depth)
    _timed(f"cab_squeeze_kernel<2, {name}>", 2.0 * B * H * W * 9 * C_ * 3, lambda: _lib.check(
        lib.hat_conv3x3_to_yuv(_ptr(x), _ptr(wpk), _ptr(bias8), C.byref(surf), B, H, W, C_, ldx, y.shape[1], y.shape[2], out_scale, m4, m, dtype,
                               _stream()), "hat_conv3x3_to_yuv"), tag=f"k3 {C_}->3 {H}x{W} row sweep {name}")


def upfold_to_yuv(x, pf, y, cb, cr, *, sub, B: int, H: int, W: int, ldx: int, out_scale: float, mean, from_rgb, dtype: int, depth: int = 8,
                  msb=False):
    """The folded ending with the YCbCr conversion of any subsampling (or grey) as its epilogue: planes_to_yuv of what
    upfold_to_planes writes, cropped to the top-left h x w pixels of the views; no fp32 image is written (hat_upfold_to_yuv)."""
    lib = _lib.load()
    surf = yuv_surface(y, cb, cr, sub=sub, depth=depth, msb=msb, what="upfold_to_yuv")
    if y.shape[0] != B:
        raise RuntimeError(f"upfold_to_yuv: destination batch {y.shape[0]} != {B}")
    m, name = _f12(from_rgb), _sub_name(sub, depth)
    _timed(f"upfold_kernel<{name}>", _upfold_flops(B, H, W), lambda: _lib.check(
        lib.hat_upfold_to_yuv(_ptr(x), _ptr(pf.w), _ptr(pf.bias), C.byref(surf), B, H, W, ldx, y.shape[1], y.shape[2], out_scale, float(mean[0]),
                              float(mean[1]), float(mean[2]), m, dtype, _stream()), "hat_upfold_to_yuv"),
        tag=f"k5 64->2x2x3 {H}x{W} folded {name}", nbytes=_upfold_bytes(B, H, W, B * y.shape[1] * y.shape[2] * 2))


def packed_surface(frame, fmt: str, *, width=None, depth=None, msb=None, what: str = "packed_surface"):
    """(HatPackedSurface, h, w) of frame (B, h, row): device frames in the packed 4:2:2 layout `fmt` of yuv.PACKED_FORMATS, uint8
    (uyvy, yuy2, v210) or uint16 (y210) with unit-step rows of yuv.packed_shape's length; rows and frames may be pitched (a view of a
    larger tensor).  width: required for v210, checked otherwise.  The struct holds a raw pointer: keep `frame` alive while it is used."""
    from . import yuv as _yuv
    dt, depth, msb = _yuv.packed_container(fmt, depth, msb)
    tdt = torch.uint8 if dt is np.uint8 else torch.uint16
    if not isinstance(frame, torch.Tensor) or frame.dim() != 3 or frame.dtype != tdt:
        raise TypeError(f"{what} needs (B,h,row) {str(tdt)[6:]} {fmt} frames, got {getattr(frame, 'dtype', type(frame))} {tuple(getattr(frame, 'shape', ()))}")
    if not frame.is_cuda or frame.stride(2) != 1:
        raise RuntimeError("HAT HIP ops need device tensors with unit-step rows (no CPU path exists)")
    h, w = _yuv.packed_size(frame.shape, fmt, width)
    n = frame.element_size()
    s = _lib.HatPackedSurface(base=frame.data_ptr(), pitch=n * frame.stride(1), bstride=n * frame.stride(0), layout=_yuv.PACKED_FORMATS.index(fmt),
                              depth=depth, msb=int(msb))
    return s, h, w


def packed422_to_planes(frame, dst, to_rgb, *, fmt: str, width=None, depth=None, msb=None, siting: str = "center"):
    """frame (B,h,row) in the packed 4:2:2 layout `fmt` (packed_surface) -> dst (B,3,Hp,Wp) fp32 RGB planes, rows and columns past
    (h, w) filled by reflection: yuv.packed_to_planes' conversion (hat_packed422_to_planes)."""
    lib = _lib.load()
    eff, code = _siting((1, 0), siting)
    surf, h, w = packed_surface(frame, fmt, width=width, depth=depth, msb=msb, what="packed422_to_planes")
    B = frame.shape[0]
    if dst.dtype != torch.float32 or dst.dim() != 4 or dst.shape[0] != B or dst.shape[1] != 3 or dst.shape[2] < h or dst.shape[3] < w \
            or dst.device != frame.device or not dst.is_contiguous():
        raise RuntimeError(f"packed422_to_planes needs a contiguous (B,3,Hp>=h,Wp>=w) fp32 destination on {frame.device}, got "
                           f"{tuple(dst.shape)} {dst.dtype} on {dst.device} for {B} frames of {h}x{w}")
    m = _f12(to_rgb)
    _timed(f"packed422_to_planes_kernel<{fmt}, {eff}>", 0.0, lambda: _lib.check(
        lib.hat_packed422_to_planes(C.byref(surf), code, _ptr(dst), B, h, w, dst.shape[2], dst.shape[3], m, _stream()), "hat_packed422_to_planes"),
        tag=f"{fmt} {eff} {h}x{w} -> planes {dst.shape[2]}x{dst.shape[3]}")


def planes_to_packed422(src, frame, from_rgb, *, fmt: str, width=None, depth=None, msb=None, siting: str = "center"):
    """src (B,3,Hs,Ws) fp32 planes -> the top-left h x w pixels as frame (B,h,row) in the packed 4:2:2 layout `fmt` (packed_surface),
    converted as yuv.planes_to_packed converts (hat_planes_to_packed422).  Bytes of a pitched row past the layout's row are not written."""
    lib = _lib.load()
    eff, code = _siting((1, 0), siting)
    surf, h, w = packed_surface(frame, fmt, width=width, depth=depth, msb=msb, what="planes_to_packed422")
    B = frame.shape[0]
    if src.dim() != 4 or src.shape[0] != B or src.shape[1] != 3 or src.dtype != torch.float32 or src.device != frame.device or not src.is_contiguous():
        raise RuntimeError(f"planes_to_packed422 needs contiguous (B,3,Hs,Ws) fp32 planes on {frame.device}, got {tuple(src.shape)} "
                           f"{src.dtype} on {src.device}")
    m = _f12(from_rgb)
    _timed(f"planes_to_packed422_kernel<{fmt}, {eff}>", 0.0, lambda: _lib.check(
        lib.hat_planes_to_packed422(_ptr(src), B, src.shape[2], src.shape[3], C.byref(surf), code, h, w, m, _stream()), "hat_planes_to_packed422"),
        tag=f"planes {src.shape[2]}x{src.shape[3]} -> {fmt} {eff} {h}x{w}")


class FrameSide:
    """One side of a YCbCr frame call, resolved once: the layout `fmt` (yuv.LAYOUTS: planes and semi-planes; yuv.PACKED_FORMATS: packed
    4:2:2), its sample depth, word alignment and chroma siting.  The ONE place that tells the two kinds of layout apart: frame entry
    points ask it for the frame's dtype, size and shape, have it fill the planes from a frame (to_planes) and write a frame from
    planes (from_planes); `fusable` says whether the kernels that end a network have an epilogue for it (views: their destination)."""

    def __init__(self, fmt: str, *, depth: int = 8, msb=None, siting: str = "center"):
        from . import yuv as _yuv
        self.fmt, self.packed = fmt, fmt in _yuv.PACKED_FORMATS
        _yuv.check_siting(siting)
        if self.packed:
            dt, self.depth, self.msb = _yuv.packed_container(fmt, depth, msb)
            self.sub = (1, 0)
        else:
            sub_x, sub_y, _ = _yuv.check_layout(fmt)
            dt, _, _, shift = _yuv.container(depth, fmt, msb)
            self.depth, self.msb, self.sub = int(depth), bool(shift), None if sub_x is None else (sub_x, sub_y)
        self.dtype = torch.uint8 if dt is np.uint8 else torch.uint16
        self.siting = _siting(self.sub, siting)[0]
        self.fusable = not self.packed and self.siting == "center"

    def size(self, shape, width=None):
        """(h, w) of a frame array of this layout; width: required for v210, checked for every other layout."""
        from . import yuv as _yuv
        if self.packed:
            return _yuv.packed_size(shape, self.fmt, width)
        h, w = _yuv.frame_size_fmt(shape, self.fmt)
        if width is not None and int(width) != w:
            raise ValueError(f"width={width} does not agree with a {self.fmt} frame of {tuple(shape)}: its rows hold {w} pixels")
        return h, w

    def shape(self, h: int, w: int):
        from . import yuv as _yuv
        return _yuv.packed_shape(h, w, self.fmt) if self.packed else _yuv.frame_shape_fmt(h, w, self.fmt)

    def size_refusal(self, h: int, w: int):
        """None if an h x w frame exists in this layout, else the axes that would have to be even, as words."""
        sx, sy = (0, 0) if self.sub is None else self.sub
        odd = [n for n, bad in (("width", sx and w % 2), ("height", sy and h % 2)) if bad]
        return " and an even ".join(odd) if odd else None

    def rows_packed(self, t) -> bool:
        """t (B, rows, cols) lies in the standard contiguous layout (rows one row apart)."""
        return t.stride(2) == 1 and t.stride(1) == t.shape[2]

    def contiguous(self, frame):
        if self.rows_packed(frame):
            return frame
        return frame.contiguous() if frame.dtype is torch.uint8 else frame.view(torch.int16).contiguous().view(torch.uint16)

    def out(self, out, shape, dev):
        """The result tensor of `shape`: the caller's `out` (checked) or a fresh one."""
        if out is None:
            return torch.empty(shape, dtype=self.dtype, device=dev)
        if not isinstance(out, torch.Tensor) or out.dtype != self.dtype or tuple(out.shape) != tuple(shape) or out.device != dev \
                or not self.rows_packed(out):
            raise RuntimeError(f"out must be a {tuple(shape)} {str(self.dtype)[6:]} tensor on {dev} with packed rows, got "
                               f"{tuple(getattr(out, 'shape', ()))} {getattr(out, 'dtype', type(out))} on {getattr(out, 'device', None)}")
        return out

    def views(self, frame):
        return yuv_views(frame, self.fmt)

    def to_planes(self, frame, x, to_rgb, *, width=None):
        """x (B,3,Hp,Wp) fp32 = the reflect-padded RGB planes of `frame`."""
        frame = self.contiguous(frame)
        if self.packed:
            return packed422_to_planes(frame, x, to_rgb, fmt=self.fmt, width=width, depth=self.depth, msb=self.msb, siting=self.siting)
        yuv_to_planes(*self.views(frame), x, to_rgb, sub=self.sub, depth=self.depth, msb=self.msb, siting=self.siting)

    def from_planes(self, planes, frame, from_rgb, *, width=None):
        """frame = the top-left pixels of the fp32 planes, as many as `frame` holds."""
        if self.packed:
            return planes_to_packed422(planes, frame, from_rgb, fmt=self.fmt, width=width, depth=self.depth, msb=self.msb, siting=self.siting)
        planes_to_yuv(planes, *self.views(frame), from_rgb, sub=self.sub, depth=self.depth, msb=self.msb, siting=self.siting)


def u8_metrics_flags(*, y_channel: bool, bgr: bool, psnr: bool, ssim: bool) -> int:
    return (_lib.METRICS_Y if y_channel else 0) | (_lib.METRICS_BGR if bgr else 0) | (_lib.METRICS_PSNR if psnr else 0) \
        | (_lib.METRICS_SSIM if ssim else 0)


def u8_metrics_workspace_bytes(B: int, h: int, w: int, *, crop_border: int, y_channel: bool, bgr: bool = False, psnr: bool = True,
                               ssim: bool = True) -> int:
    """Bytes of workspace hat_u8_metrics needs for (B,h,w,3) frames; raises for sizes it refuses (a pure host query)."""
    lib = _lib.load()
    n = C.c_int64(0)
    _lib.check(lib.hat_u8_metrics_workspace_bytes(B, h, w, crop_border, u8_metrics_flags(y_channel=y_channel, bgr=bgr, psnr=psnr, ssim=ssim),
                                                  C.byref(n)), "hat_u8_metrics_workspace_bytes")
    return n.value


def u8_metrics(a, b, sums, workspace, *, crop_border: int, y_channel: bool, bgr: bool = False, psnr: bool = True, ssim: bool = True):
    """a, b (B, h, w, 3) uint8 (rows may be pitched) -> sums (B, 4) float64: the sum of squared differences and the SSIM-map
    sums of channel 0, 1, 2 (hat_u8_metrics; metrics_device.finalize turns them into PSNR / SSIM).  workspace: a uint8
    device tensor of at least u8_metrics_workspace_bytes(...) bytes."""
    lib = _lib.load()
    for t in (a, b):
        if t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8 or t.stride(-1) != 1 or t.stride(-2) != 3:
            raise RuntimeError("u8_metrics needs (B,h,w,3) uint8 frames with interleaved pixels")
        if not t.is_cuda:
            raise RuntimeError("HAT HIP ops need device tensors (no CPU path exists)")
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"u8_metrics needs two frames of one shape on one device, got {tuple(a.shape)} on {a.device} and "
                           f"{tuple(b.shape)} on {b.device}")
    B, h, w, _ = a.shape
    if sums.dtype != torch.float64 or tuple(sums.shape) != (B, 4) or sums.device != a.device or workspace.device != a.device:
        raise RuntimeError(f"u8_metrics needs a (B,4) float64 destination and a workspace on {a.device}")
    need = u8_metrics_workspace_bytes(B, h, w, crop_border=crop_border, y_channel=y_channel, bgr=bgr, psnr=psnr, ssim=ssim)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.data_ptr() % 8:
        raise RuntimeError(f"u8_metrics needs an 8-byte aligned uint8 workspace of at least {need} bytes")
    flags = u8_metrics_flags(y_channel=y_channel, bgr=bgr, psnr=psnr, ssim=ssim)
    nch = 1 if y_channel else 3
    hc, wc = h - 2 * crop_border, w - 2 * crop_border
    flops = 2.0 * B * nch * (hc - 10) * (wc - 10) * 5 * 22 if ssim else 0.0
    _timed(f"u8_metrics_kernel<{'y' if y_channel else 'rgb'}>", flops, lambda: _lib.check(
        lib.hat_u8_metrics(a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0), B, h, w, crop_border, flags,
                           _ptr(sums), _ptr(workspace), _stream()), "hat_u8_metrics"),
        tag=f"u8 metrics {h}x{w} crop {crop_border}{' psnr' if psnr else ''}{' ssim' if ssim else ''}", nbytes=2.0 * B * h * w * 3)


# ---- NIQE block sums (definition: niqe.py; kernels: csrc/hat_niqe.hip) ----
_niqe_buffers = {}   # (device, B, h, w, crop_border) -> the workspace's four views, the two stats tensors, the window


def niqe_workspace(B: int, h: int, w: int, *, crop_border: int):
    """(H96, W96, bytes) of hat_niqe_workspace_bytes for (B,h,w,3) frames; raises for sizes it refuses (a pure host query)."""
    lib = _lib.load()
    H, W, n = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    _lib.check(lib.hat_niqe_workspace_bytes(B, h, w, crop_border, C.byref(H), C.byref(W), C.byref(n)), "hat_niqe_workspace_bytes")
    return H.value, W.value, n.value


def _niqe_buffers_for(dev, B, h, w, crop_border):
    import numpy as np

    from . import niqe as _nq
    key = (str(dev), B, h, w, crop_border)
    buf = _niqe_buffers.get(key)
    if buf is None:
        H, W, nbytes = niqe_workspace(B, h, w, crop_border=crop_border)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        px, views, o = B * H * W, [], 0
        for shape in ((B, H, W), (B, H, W), (B, H // 2, W), (B, H // 2, W // 2)):
            n = shape[0] * shape[1] * shape[2]
            views.append(ws[o:o + n].view(shape))
            o += n
        assert o * 4 == nbytes and px == views[0].numel()
        win = np.ascontiguousarray(_nq.gaussian_window(), dtype=np.float64)
        buf = _niqe_buffers[key] = {"plane": views[0], "unit": views[1], "mid": views[2], "half": views[3], "window": win,
                                    "stats96": torch.zeros(B, H // 96, W // 96, 25, dtype=torch.float64, device=dev),
                                    "stats48": torch.zeros(B, H // 96, W // 96, 25, dtype=torch.float64, device=dev)}
    return buf


def niqe_stats(frame_u8, *, crop_border: int, bgr: bool = False):
    """frame_u8: (h,w,3) or (B,h,w,3) uint8 device frames (rows may be pitched) -> (stats96, stats48): (B, H96 / 96, W96 / 96, 25)
    float64 device tensors, niqe.stats_of(niqe.y_plane(frame, crop_border), acc=float64) per sample.  Five launches (Y, the two
    resize passes, the two block kernels); the buffers are kept per shape and the tensors returned are those buffers: the next
    call of the same shape overwrites them."""
    lib = _lib.load()
    f = frame_u8
    if not isinstance(f, torch.Tensor) or not f.is_cuda:
        raise RuntimeError("niqe_stats needs a uint8 device tensor (no CPU path exists: niqe.stats_of is the host definition)")
    if f.dim() == 3:
        f = f.unsqueeze(0)
    if f.dim() != 4 or f.shape[3] != 3 or f.dtype != torch.uint8 or f.stride(3) != 1 or f.stride(2) != 3:
        raise RuntimeError(f"niqe_stats needs (B,h,w,3) uint8 frames with interleaved pixels, got {tuple(frame_u8.shape)} {frame_u8.dtype}")
    B, h, w, _ = f.shape
    crop_border = int(crop_border)
    dev = f.device
    buf = _niqe_buffers_for(dev, B, h, w, crop_border)
    plane, unit, mid, half = buf["plane"], buf["unit"], buf["mid"], buf["half"]
    H, W = plane.shape[1], plane.shape[2]
    th, tw = _resize_axis(dev, H, 0.5, True), _resize_axis(dev, W, 0.5, True)
    if th["out"] != H // 2 or tw["out"] != W // 2:
        raise RuntimeError(f"niqe_stats: the half size of {H}x{W} came out as {th['out']}x{tw['out']}")
    win = buf["window"].ctypes.data_as(C.POINTER(C.c_double))
    st = _stream()
    _timed("niqe_y_kernel", 0.0, lambda: _lib.check(
        lib.hat_niqe_y_u8(f.data_ptr(), f.stride(1), f.stride(0), B, h, w, crop_border, int(bgr), _ptr(plane), _ptr(unit), st), "hat_niqe_y_u8"),
        tag=f"niqe Y {h}x{w} crop {crop_border} -> {H}x{W}", nbytes=B * (3.0 * H * W + 8.0 * H * W))
    _timed("plane_rows_kernel", 2.0 * B * (H // 2) * W * th["P"], lambda: _lib.check(
        lib.hat_imresize_plane_rows(_ptr(unit), _ptr(mid), B, H, W, H // 2, _ptr(th["w"]), _ptr(th["src"]), th["P"], th["w"].numel(), st),
        "hat_imresize_plane_rows"), tag=f"niqe half rows {H}x{W}", nbytes=B * 4.0 * (H * W + H // 2 * W))
    _timed("plane_cols_kernel", 2.0 * B * (H // 2) * (W // 2) * tw["P"], lambda: _lib.check(
        lib.hat_imresize_plane_cols(_ptr(mid), B, H // 2, W, W // 2, _ptr(tw["w"]), _ptr(tw["src"]), tw["P"], tw["w"].numel(), 255.0,
                                    _ptr(half), st), "hat_imresize_plane_cols"),
        tag=f"niqe half cols {H // 2}x{W}", nbytes=B * 4.0 * (H // 2 * W + H // 2 * (W // 2)))
    for src, block, out in ((plane, 96, buf["stats96"]), (half, 48, buf["stats48"])):
        hh, ww = src.shape[1], src.shape[2]
        _timed(f"niqe_block_kernel<{block}>", 4.0 * 49 * 2 * B * hh * ww, lambda: _lib.check(
            lib.hat_niqe_block_stats(_ptr(src), B, hh, ww, block, win, _ptr(out), st), "hat_niqe_block_stats"),
            tag=f"niqe blocks {block} {hh}x{ww}", nbytes=B * (4.0 * hh * ww + 200.0 * (hh // block) * (ww // block)))
    return buf["stats96"], buf["stats48"]


def cab_squeeze_units(H: int, W: int) -> int:
    lib = _lib.load()
    rows, units = C.c_int32(0), C.c_int32(0)
    _lib.check(lib.hat_cab_squeeze_units(H, W, C.byref(rows), C.byref(units)), "hat_cab_squeeze_units")
    return units.value


def cab_squeeze(x, wpk, bias8, out, colsum, *, B: int, H: int, W: int, C_: int, ldx: int, dtype: int):
    lib = _lib.load()
    _timed("cab_squeeze_kernel", 2.0 * B * H * W * 9 * C_ * 6, lambda: _lib.check(
        lib.hat_cab_squeeze(_ptr(x), _ptr(wpk), _ptr(bias8), _ptr(out), _ptr(colsum), B, H, W, C_, ldx, dtype, _stream()),
        "hat_cab_squeeze"), tag=f"k3 {C_}->8 {H}x{W} row sweep")


def window_attention(q, kv, bias_flip, out, *, B: int, H: int, W: int, C_: int, heads: int, ws: int, shift: int, ldq: int,
                     ldkv: int, ldo: int, dtype: int):
    """(S)W-MSA core (hat_window_attention; swinir_arch.py:147-168 + roll / partition / mask / reverse :291-317)."""
    lib = _lib.load()
    # (an unknown dtype code is the library's to refuse, like every other argument)
    _timed(f"ocab_attn_kernel<{_TNAME.get(dtype, dtype)}, self>", 2.0 * 2 * ws * ws * C_ * B * H * W, lambda: _lib.check(
        lib.hat_window_attention(_ptr(q), _ptr(kv), _ptr(bias_flip), _ptr(out), B, H, W, C_, heads, ws, shift, ldq, ldkv, ldo,
                                 dtype, _stream()), "hat_window_attention"))


# ------------------------------------------------------------------------------------------------
# fused feed-forward half of the HAB (hat_ffn)
# ------------------------------------------------------------------------------------------------
def ffn_supported(C_: int) -> bool:
    """Shapes hat_ffn is instantiated for (anything else uses the unfused kernels)."""
    return C_ in (144, 180) or (C_ <= 32 and C_ % 32 != 16 and C_ >= 8)


def ffn2_supported(C_: int, hid: int, dtype: int) -> bool:
    """Shapes hat_ffn2 (fp16 hidden tensor, VALU depthwise conv) is built for."""
    return C_ == 144 and hid % 32 == 0 and dtype == HAT_BF16


def tail3_supported(C_: int, hid: int, dtype: int) -> bool:
    """Shapes hat_hab_tail3 is built for: embed_dim 144 (hidden 288, folded CAB) and 180 (hidden 360 padded to 384, c2 as a map)."""
    return dtype == HAT_BF16 and ((C_ == 144 and hid % 32 == 0) or (C_ == 180 and hid == 360))


def _ffn_desc(pf: PackedFFN, B, H, W, dtype):
    d = HatFfnDesc()
    d.B, d.H, d.W, d.C, d.chunks, d.dtype = B, H, W, pf.C, pf.chunks, dtype
    return d


def ffn_tiles(pf: PackedFFN, H: int, W: int, dtype: int) -> int:
    lib = _lib.load()
    d = _ffn_desc(pf, 1, H, W, dtype)
    n = C.c_int32(0)
    _lib.check(lib.hat_ffn_tiles(C.byref(d), C.byref(n)), "hat_ffn_tiles")
    return n.value


def ffn_m_ld(C_: int) -> int:
    """Row length (elements) of the pre-normalised input image hat_ffn's m_in expects: [LN (C) | 1.0 | zeros]."""
    return (C_ + 1 + 31) // 32 * 32


def _fill_ffn(d, pf: PackedFFN, t_in, t_out, ln_g, ln_b, ln1, n_out, ldn, gap_out, gap_c, m_in=None, ldm_in=0, n16_out=None):
    d.t_in, d.t_out, d.ln_g, d.ln_b = _ptr(t_in), _ptr(t_out), _ptr(ln_g), _ptr(ln_b)
    if m_in is not None:
        d.m_in, d.ldm_in = _ptr(m_in), ldm_in
    d.w1f, d.b1, d.dww, d.dwb, d.w2f, d.b2 = _ptr(pf.w1f), _ptr(pf.b1), _ptr(pf.dww), _ptr(pf.dwb), _ptr(pf.w2f), _ptr(pf.b2)
    if ln1 is not None:
        d.ln1_g, d.ln1_b, d.n_out, d.ldn = _ptr(ln1[0]), _ptr(ln1[1]), _ptr(n_out), ldn
        d.gap_out, d.gap_c = (_ptr(gap_out) if gap_c else None), gap_c
        d.n16_out = _ptr(n16_out)


def ffn(pf: PackedFFN, t_in, t_out, ln_g, ln_b, *, B: int, H: int, W: int, dtype: int, ln1=None, n_out=None, ldn: int = 0,
        gap_out=None, gap_c: int = 0, m_in=None, ldm_in: int = 0):
    lib = _lib.load()
    d = _ffn_desc(pf, B, H, W, dtype)
    _fill_ffn(d, pf, t_in, t_out, ln_g, ln_b, ln1, n_out, ldn, gap_out, gap_c, m_in, ldm_in)
    flops = B * H * W * (2.0 * pf.C * 2 * pf.hid + 2.0 * 9 * 2 * pf.hid + 2.0 * pf.hid * pf.C)
    # algorithmic HBM bytes per pixel: t_in read once (fp32), t_out written (fp32), the next block's LayerNorm output
    # written (T); weights and the on-chip hidden tensor do not count
    es = 2 if dtype == HAT_BF16 else 4
    # (with m_in, LayerNorm2(t_in) arrives pre-computed as T rows: it replaces the haloed fp32 read; t_in is still read
    # once for the residual)
    nbytes = B * H * W * (4.0 * pf.C + 4.0 * pf.C + (es * ldn if ln1 is not None else 0) + (es * ldm_in if m_in is not None else 0))
    if pf.layout == "tail3":
        raise RuntimeError("a hat_hab_tail3-packed FFN has no stand-alone launch: pack with pack_ffn2 for hat_ffn2")
    if pf.layout == "ffn2":
        _timed("ffn2_kernel", flops, lambda: _lib.check(lib.hat_ffn2(C.byref(d), _stream()), "hat_ffn2"), nbytes=nbytes)
        return
    _timed(f"ffn_kernel<{_TNAME[dtype]}>", flops, lambda: _lib.check(lib.hat_ffn(C.byref(d), _stream()), "hat_ffn"),
           nbytes=nbytes)


def hab_tail_supported(pf: PackedFFN, aggr: PackedConv, mid: int, dtype: int) -> bool:
    if pf.C == 180:   # hat_hab_tail3 with the CAB's c2 as a map (no fold: mid is 60)
        return pf.layout == "tail3" and aggr.frag and aggr.nt == 12 and aggr.n_slices == 1 and aggr.kpad == 192 and dtype == HAT_BF16
    return pf.layout in ("ffn2", "tail3") and aggr.frag and aggr.nt == 9 and aggr.n_slices == 1 and aggr.kpad == 160 and mid <= 8 and dtype == HAT_BF16


def hab_tail(pf: PackedFFN, aggr: PackedConv, t_in, t_out, ln_g, ln_b, *, n, ldn_in: int, y16, c1=None, wf=None, bias_b, B: int, H: int,
             W: int, dtype: int, ln1=None, n_out=None, ldn: int = 0, gap_out=None, gap_c: int = 0, n16_out=None,
             r2=None, ldr2: int = 0, r2scale=None, r2scale_bstride: int = 0, sat=None):
    """hat_hab_tail: aggregation + folded CAB + residuals + the whole gated FFN in one launch (t_in = the residual stream
    BEFORE the aggregation).  hat_hab_tail3 at embed_dim 144 takes t_in / t_out as fp32 or FP16 rows (by the tensors' dtype).
    sat: the FP16-range guard's slot: hat_hab_tail3_guarded instead of hat_hab_tail3, for an FP16 t_out only."""
    lib = _lib.load()
    h = HatHabTailDesc()
    d = h.ffn
    d.B, d.H, d.W, d.C, d.chunks, d.dtype = B, H, W, pf.C, pf.chunks, dtype
    _fill_ffn(d, pf, t_in, t_out, ln_g, ln_b, ln1, n_out, ldn, gap_out, gap_c, n16_out=n16_out)
    h.n, h.y16, h.c1, h.w_aggr, h.wf, h.bias_b, h.ldn_in = _ptr(n), _ptr(y16), _ptr(c1), _ptr(aggr.w), _ptr(wf), _ptr(bias_b), ldn_in
    h.r2, h.ldr2, h.r2scale, h.r2scale_bstride = _ptr(r2), ldr2, _ptr(r2scale), r2scale_bstride
    in_half, out_half = t_in.dtype == torch.float16, t_out.dtype == torch.float16
    if (in_half or out_half) and not (pf.C == 144 and pf.layout == "tail3"):
        raise RuntimeError("an FP16 residual stream is only instantiated for hat_hab_tail3 at embed_dim 144")
    if (not in_half and t_in.dtype != torch.float32) or (not out_half and t_out.dtype != torch.float32):
        raise RuntimeError("hab_tail: t_in / t_out must be fp32 or FP16 rows")
    h.reserved1 = (1 if in_half else 0) | (2 if out_half else 0)
    if sat is not None and not (pf.layout == "tail3"):
        raise RuntimeError("the FP16-range guard is hat_hab_tail3's")
    tail3 = (lambda: lib.hat_hab_tail3(C.byref(h), _stream())) if sat is None else (lambda: lib.hat_hab_tail3_guarded(C.byref(h), _sat_ptr(sat), _stream()))
    what = "hat_hab_tail3" if sat is None else "hat_hab_tail3_guarded"
    if pf.C == 180:   # aggregation + c2 term + FFN; n, y16, c2 (T), t read once, t_out and the next LayerNorm written
        flops = B * H * W * (2.0 * pf.C * pf.C + 2.0 * pf.C * 2 * pf.hid + 2.0 * 9 * 2 * pf.hid + 2.0 * pf.hid * pf.C)
        nbytes = B * H * W * (2.0 * ldn_in + 32 + 2.0 * ldr2 + 4.0 * pf.C + 4.0 * pf.C + (2 * ldn if ln1 is not None else 0))
        _timed("tail3l_kernel", flops, lambda: _lib.check(tail3(), what), nbytes=nbytes)
        return
    flops = B * H * W * (2.0 * pf.C * (pf.C + 72) + 2.0 * pf.C * 2 * pf.hid + 2.0 * 9 * 2 * pf.hid + 2.0 * pf.hid * pf.C)
    # algorithmic HBM bytes per pixel: n (T), y16 (T x 16), c1 (T x 8), t (fp32) read once; t_out (fp32) and the next
    # block's LayerNorm output (T) written
    nbytes = B * H * W * (2.0 * ldn_in + 32 + 16 + (2.0 if in_half else 4.0) * pf.C + (2.0 if out_half else 4.0) * pf.C + (2 * ldn if ln1 is not None else 0))
    if pf.layout == "tail3":
        _timed("tail3_kernel", flops, lambda: _lib.check(tail3(), what), nbytes=nbytes)
        return
    _timed("ffn2_kernel<aggr>", flops, lambda: _lib.check(lib.hat_hab_tail(C.byref(h), _stream()), "hat_hab_tail"), nbytes=nbytes)


# ------------------------------------------------------------------------------------------------
# pointwise linear layers (hat_linear): fragment-packed weights, weight-stationary streaming GEMM
# ------------------------------------------------------------------------------------------------
_PW_SHAPES = {(9, 5), (18, 5), (9, 9), (12, 6), (23, 6), (12, 12), (4, 1), (4, 2)}  # (nt, ceil(Cin/32)) instantiated in hat_pw.hip


def linear_supported(nout: int, cin: int, dtype: int) -> bool:
    nt, _ = choose_nt_linear(nout, cin, dtype)
    ks = -(-cin // 32)
    lds = nt * ks * 64 * 8 * (2 if dtype == HAT_BF16 else 4)
    return (nt, ks) in _PW_SHAPES and lds <= 163840 and cin % 4 == 0


def linear(pw: PackedConv, x: torch.Tensor, out: torch.Tensor, *, B: int, H: int, W: int, dtype: int, ldx: int, ldo: int,
           out_mode: int = O_NHWC_T, act: int = ACT_NONE, n_store: Optional[int] = None, x0: Optional[torch.Tensor] = None,
           c_split: int = 0, ldx0: int = 0, r1: Optional[torch.Tensor] = None, ldr1: int = 0, r2: Optional[torch.Tensor] = None,
           ldr2: int = 0, r2scale: Optional[torch.Tensor] = None, r2scale_bstride: int = 0, ln=None,
           ln_out: Optional[torch.Tensor] = None, ld_ln: int = 0, ln_ones: bool = False, sat: Optional[torch.Tensor] = None):
    """ln=(gamma, beta), ln_out, ld_ln: also emit LayerNorm(result) as T rows (hat_linear's fused LayerNorm; needs a
    residual operand); ln_ones appends the [1.0, 0...] tail that hat_ffn's m_in expects.
    sat: the FP16-range guard's slot: hat_linear_guarded instead of hat_linear, for FP16 output rows only."""
    lib = _lib.load()
    d = HatConvDesc()
    d.x, d.x0, d.w, d.bias, d.out = _ptr(x), _ptr(x0), _ptr(pw.w), _ptr(pw.bias), _ptr(out)
    d.r1, d.r2, d.r2scale = _ptr(r1), _ptr(r2), _ptr(r2scale)
    if ln is not None:
        d.ln_g, d.ln_b, d.ln_out, d.ld_ln, d.ln_ones = _ptr(ln[0]), _ptr(ln[1]), _ptr(ln_out), ld_ln, int(ln_ones)
    d.B, d.H, d.W, d.Cin, d.ldx, d.x_mode = B, H, W, pw.cin, ldx, X_NHWC_T
    d.c_split, d.ldx0, d.ksize, d.Kpad, d.nt, d.n_slices = c_split, ldx0, 1, pw.kpad, pw.nt, pw.n_slices
    d.n_store = pw.nout if n_store is None else n_store
    d.ldo, d.out_mode, d.act, d.ldr1, d.ldr2, d.r2scale_bstride, d.dtype = ldo, out_mode, act, ldr1, ldr2, r2scale_bstride, dtype
    d.reserved0 = _stream16(r1, out, out_mode)
    flops = 2.0 * B * H * W * pw.cin * pw.nout
    _timed(f"pw_kernel<{_TNAME[dtype]}, {pw.nt}, {pw.kpad // 32}>", flops,
           lambda: _lib.check(lib.hat_linear(C.byref(d), _stream()) if sat is None else lib.hat_linear_guarded(C.byref(d), _sat_ptr(sat), _stream()),
                              f"hat_linear{'' if sat is None else '_guarded'}(Cin={pw.cin}, N={pw.nout})"),
           tag=f"lin {pw.cin}->{pw.nout} {H}x{W} o{out_mode}{' r1' if r1 is not None else ''}{' r2' if r2 is not None else ''}")


_T3_SHAPES = {(1, 144), (9, 8), (1, 24), (4, 8)}  # (nt, Cin_p) instantiated in tap3_kernel


def conv3x3_small_supported(nout: int, cin: int, dtype: int = HAT_BF16) -> bool:
    nt, n_slices = choose_nt(nout)
    cin_p = (cin + 7) // 8 * 8
    lds = nt * (-(-9 * cin_p // 32)) * 64 * 8 * (2 if dtype == HAT_BF16 else 4)
    return (nt, cin_p) in _T3_SHAPES and n_slices == 1 and lds <= 81920


def _c3_desc(pw, B, H, W, dtype, ldx):
    d = HatConvDesc()
    d.B, d.H, d.W, d.Cin, d.ldx, d.x_mode = B, H, W, pw.cin, ldx, X_NHWC_T
    d.ksize, d.Kpad, d.nt, d.n_slices, d.dtype = 3, pw.kpad, pw.nt, 1, dtype
    return d


def conv3x3_small_groups(pw: PackedConv, B: int, H: int, W: int, dtype: int) -> int:
    lib = _lib.load()
    d = _c3_desc(pw, B, H, W, dtype, 8)
    n = C.c_int32(0)
    _lib.check(lib.hat_conv3x3_small_groups(C.byref(d), C.byref(n)), "hat_conv3x3_small_groups")
    return n.value


def conv3x3_small(pw: PackedConv, x, out, *, B: int, H: int, W: int, dtype: int, ldx: int, ldo: int, act: int = ACT_NONE,
                  n_store: Optional[int] = None, out_mode: int = O_NHWC_T, colsum=None):
    lib = _lib.load()
    d = _c3_desc(pw, B, H, W, dtype, ldx)
    d.x, d.w, d.bias, d.out, d.colsum = _ptr(x), _ptr(pw.w), _ptr(pw.bias), _ptr(out), _ptr(colsum)
    d.n_store = pw.nout if n_store is None else n_store
    d.ldo, d.out_mode, d.act = ldo, out_mode, act
    flops = 2.0 * B * H * W * 9 * pw.cin * pw.nout
    _timed(f"tap3_kernel<{_TNAME[dtype]}, {pw.nt}>", flops,
           lambda: _lib.check(lib.hat_conv3x3_small(C.byref(d), _stream()), f"hat_conv3x3_small(Cin={pw.cin}, N={pw.nout})"),
           tag=f"c3s {pw.cin}->{pw.nout} {H}x{W}")


# ------------------------------------------------------------------------------------------------
# CAB expand conv + ECA folded into the ESC aggregation (hat_cab_fold + hat_aggr_cab)
# ------------------------------------------------------------------------------------------------
def aggr_cab_supported(C_: int, mid: int, dtype: int) -> bool:
    return C_ == 144 and mid <= 8 and dtype == HAT_BF16


def cab_fold(c1, c1_colsum, tiles: int, ldcs: int, w2, b2, wk, k: int, bias_in, conv_scale: float, scale, wf, bias_out, tmp, *,
             B: int, H: int, W: int, C_: int, mid: int, dtype: int, stats=None, w2f=None):
    """stats: (B, >= 72) fp32 = the frame-wide sums of c1 ([total 8 | first row | last row | first column | last column | four
    corner pixels]); H, W are then the FULL frame's and c1 / c1_colsum are not read (band-sharded frames)."""
    lib = _lib.load()
    d = HatCabFoldDesc()
    d.stats = _ptr(stats)
    d.w2f = _ptr(w2f)
    d.c1, d.c1_colsum, d.w2, d.b2, d.wk, d.bias_in = _ptr(c1), _ptr(c1_colsum), _ptr(w2), _ptr(b2), _ptr(wk), _ptr(bias_in)
    d.scale, d.wf, d.bias_out, d.tmp = _ptr(scale), _ptr(wf), _ptr(bias_out), _ptr(tmp)
    d.B, d.H, d.W, d.C, d.mid, d.ld1, d.tiles, d.ldcs, d.k, d.ld_scale, d.dtype = B, H, W, C_, mid, 8, tiles, ldcs, k, scale.shape[1], dtype
    d.conv_scale = conv_scale
    _timed("cab_fold", 0.0, lambda: _lib.check(lib.hat_cab_fold(C.byref(d), _stream()), "hat_cab_fold"))


def aggr_cab(pw: PackedConv, x, out, c1, wf, bias_b, *, B: int, H: int, W: int, dtype: int, ldx: int, ldo: int, x0=None,
             c_split: int = 0, ldx0: int = 0, r1=None, ldr1: int = 0):
    lib = _lib.load()
    dd = HatAggrCabDesc()
    d = dd.lin
    d.x, d.x0, d.w, d.bias, d.out, d.r1 = _ptr(x), _ptr(x0), _ptr(pw.w), _ptr(pw.bias), _ptr(out), _ptr(r1)
    d.B, d.H, d.W, d.Cin, d.ldx, d.x_mode = B, H, W, pw.cin, ldx, X_NHWC_T
    d.c_split, d.ldx0, d.ksize, d.Kpad, d.nt, d.n_slices, d.n_store = c_split, ldx0, 1, pw.kpad, pw.nt, pw.n_slices, pw.nout
    d.ldo, d.out_mode, d.act, d.ldr1, d.dtype = ldo, O_NHWC_F32, ACT_NONE, ldr1, dtype
    dd.c1, dd.wf, dd.bias_b = _ptr(c1), _ptr(wf), _ptr(bias_b)
    flops = 2.0 * B * H * W * pw.nout * (pw.cin + 9 * 8)
    _timed("aggr_cab_kernel", flops, lambda: _lib.check(lib.hat_aggr_cab(C.byref(dd), _stream()), "hat_aggr_cab"),
           tag=f"aggr+cab {pw.cin}+72->{pw.nout} {H}x{W}")
