"""HATEngine — host-side orchestration of the HIP kernels for one HAT network.

Holds the packed weights (per storage dtype) and a per-shape workspace in HBM, and enqueues the
kernel sequence of `HAT.forward` (reference: hat/archs/hat_arch.py:848-859 and the blocks it
calls; op-by-op map in SURVEY.md App. A) on the current stream.  Nothing here computes on the
CPU or through torch ops: torch only allocates device buffers and packs weights at load time.

Which kernel runs where is decided once, at pack time (_Hab, _Ocab, _Group); the forward is a driver over stage steps.
`forward`, the lock and the workspace LRU are engine_base.EngineBase's; the ensemble and the frame entry points frame_boundary.FrameBoundary's.
Data layout in HBM (B = batch, N = H*W pixels, C = embed_dim):
  residual stream      tA, tB : fp32 (B, N, C)  two buffers: tA = RHAG input/output, tB = working copy
  shallow feature      f0     : fp32 (B, N, C)
  MFMA operands        n, c2, q, ao : T (B, N, ld(C));  u : T (B, N, ld(4C));  g, kv : T (B, N, ld(2C))
                       c1 : T (B, N, ld(C/cr));  y16 : T (B, N, pdim)       ld(x) = round_up(x, 8)
  upsampler            fb : T (B, N, 64);  up_i : T (B, r^2i N, 64);  output y : fp32 (B, 3, sH, sW) NCHW
T = bf16 (performance path) or fp32 (exact-fp32 parity path).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
import warnings
from typing import Dict, Optional

import torch

from . import ops
from .engine_base import EngineBase
from .frame_boundary import FrameBoundary
from .ops import (ACT_GELU, ACT_LRELU, ACT_NONE, O_NCHW_F32, O_NHWC_F32, O_NHWC_T, O_PIXSHUF_T, X_NCHW_F32_MEAN, X_NHWC_F32, X_NHWC_T)
from .packing import _ESC

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # hat_arch.py:659


def _r8(x: int) -> int:
    return (x + 7) // 8 * 8


def _r4(x: int) -> int:
    return (x + 3) // 4 * 4


T16_GUARD_MODES = ("defer", "sync", "off")


@dataclasses.dataclass(frozen=True)
class Options:
    """The engine's environment switches, read once per process: HATEngine reads them when it is built (a switch changed later
    takes effect in the next engine built).  None is needed in production: each selects an older kernel SEQUENCE of the same
    arithmetic, for A/B runs and diagnosis.  "=1" switches take exactly "1", the others any non-empty value.
      HAT_NO_N16=1           no compact 16-channel copy of the LayerNorm rows for the 13x13 ESC conv
      HAT_NO_T16=1           the residual stream in fp32 everywhere (default on the bf16 path at embed_dim 144: FP16 rows wherever
                             every reader takes them: group conv, fused HAB tails, OCAB projection / MLP)
      HAT_NO_FUSED_FFN=1     the FFN as fc1 -> dw + gate -> fc2 instead of hat_ffn / hat_ffn2
      HAT_FFN_V1=1           hat_ffn (bf16 hidden tensor) instead of hat_ffn2
      HAT_NO_HAB_TAIL=1      no fused HAB tail: the aggregation (hat_aggr_cab / hat_linear), then the fused FFN
      HAT_NO_CAB_FOLD        CAB expand conv + ECA as their own launches instead of folded into the aggregation
      HAT_NO_CAB_SWEEP       CAB squeeze conv and conv_last on hat_conv instead of the row-sweep kernels
      HAT_NO_ESC13=1         the 13x13 ESC conv on hat_conv instead of hat_esc_conv13
      HAT_ESC_SIDE=1         the 13x13 conv (not the CAB squeeze chain) on the side stream: round 2's arrangement
      HAT_ONE_STREAM=1       no side stream: a HAB's two short chains and the q / kv projections run one after the other (what
                             hat_plan_forward replays; HATEngine.forward(x, one_stream=...) overrides it per call)
      HAT_NO_ATTN_LOG2=1     hat_ocab_attention instead of hat_ocab_attention_log2
      HAT_NO_OCAB_MLP        the OCAB MLP as two hat_linear launches instead of hat_ocab_mlp
      HAT_NO_OCAB_QKV        the OCAB q and kv projections as two hat_linear launches on two streams instead of hat_ocab_qkv
      HAT_NO_BF16_CONV_IN    fp32 rows into the group conv instead of the OCAB MLP's bf16 rows
      HAT_NO_CONV_LN         the LayerNorm after the group conv as its own launch instead of the conv's epilogue
      HAT_NO_UPFOLD=1        the last Upsample conv and conv_last as their two launches instead of hat_upfold_*
      HAT_NO_HEAD_FUSED=1    conv_first, the patch-embed LayerNorm and the first norm1 as their three launches instead of hat_head_fused
    One switch is not an A/B switch and takes a word:
      HAT_T16_GUARD          defer (default) | sync | off — what happens when the FP16 residual stream leaves the FP16 range
                             (_T16Guard below): off launches the unguarded entries and clips in silence; any other
                             word raises"""
    no_n16: bool = False
    no_t16: bool = False
    no_fused_ffn: bool = False
    ffn_v1: bool = False
    no_hab_tail: bool = False
    no_cab_fold: bool = False
    no_cab_sweep: bool = False
    no_esc13: bool = False
    esc_side: bool = False
    one_stream: bool = False
    no_attn_log2: bool = False
    no_ocab_mlp: bool = False
    no_ocab_qkv: bool = False
    no_bf16_conv_in: bool = False
    no_conv_ln: bool = False
    no_upfold: bool = False
    no_head_fused: bool = False
    t16_guard: str = "defer"

    def __post_init__(self):
        if self.t16_guard not in T16_GUARD_MODES:
            raise ValueError(f"t16_guard / HAT_T16_GUARD is one of {', '.join(T16_GUARD_MODES)}, got {self.t16_guard!r}")

    @classmethod
    def from_env(cls, env=None) -> "Options":
        """Field f is the variable HAT_<F>."""
        env = os.environ if env is None else env
        get = lambda name: env.get("HAT_" + name.upper(), "")
        any_value = ("no_cab_fold", "no_cab_sweep", "no_ocab_mlp", "no_ocab_qkv", "no_bf16_conv_in", "no_conv_ln")
        kw = {k.name: (get(k.name) != "" if k.name in any_value else get(k.name) == "1") for k in dataclasses.fields(cls) if k.type == "bool"}
        return cls(t16_guard=(get("t16_guard") or "defer"), **kw)


class _T16Guard:
    """The FP16-range guard of the residual stream: `slot`, one word on the device that the guarded launches of a
    forward raise to the bit pattern of the largest magnitude their FP16 stores clipped (0: none did); `host`, the pinned word
    it is copied to behind the last launch, and `event`, recorded behind that copy; `pending`, the forwards handed to the
    caller whose word nobody has looked at yet.  The slot is zeroed only while nothing is pending, so a word that is looked
    at late still holds the largest magnitude of every forward since the last look.  One per engine, not per workspace: every
    shape and every band of a frame raises the same word."""

    def __init__(self, dev):
        self.slot = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.pending = 0

    def word(self) -> int:
        return int(self.host[0]) & 0xFFFFFFFF


class _Packed:
    """Read access by key as well as by attribute, so callers that read the packed layers as dicts (L["habs"], hb["ffn"]) keep working."""

    def __getitem__(self, key):
        try:
            return getattr(self, key)
        except AttributeError:
            raise KeyError(key) from None


class _Hab(_Packed):
    """One HAB (hat_arch.py:217-238): packed weights and the launches chosen for it at pack time.
    fold: the CAB expand conv + ECA folded into the aggregation (hat_cab_fold / hat_aggr_cab), else None (plain CAB convs).
    tail: "fused144" (hat_hab_tail3 on ffn3) | "fused180" (hat_hab_tail3 with c2 as a map) |
          "aggr_cab" (after a fold) or "aggr" (hat_linear) followed by the FFN: fused (ffn) or fc1 / gate / fc2 (ffn None).
    next_ln: (gamma, beta), gap_c of the LayerNorm its consumer (the next HAB or the OCAB) starts with.
    out16: the fused tail hands the residual stream on as FP16 rows."""
    fold = ffn = ffn3 = fc1 = fc2 = bias256 = None
    tail = "aggr"
    next_ln = None
    out16 = False


class _Ocab(_Packed):
    """One OCAB (hat_arch.py:326-393): packed weights; qkvf / mlpf are the fused launches where they are built (else None),
    esc the OCAB-ESC on the key / value path (None without one), fh0 / fh2 HATX's saliency head."""
    qkvf = mlpf = esc = fh0 = fh2 = None


class _Naf(_Packed):
    """The NAF stem of HybridHATNAF (hybrid_hat_naf_arch.py:69-82): head / tail 3x3 convs packed for hat_conv, the blocks for
    hat_naf_half / hat_naf_fold (packing.PackedNafBlock), c = naf_width."""

    def __init__(self, c, head, blocks, tail):
        self.c, self.head, self.blocks, self.tail = c, head, blocks, tail


class _Group(_Packed):
    """One residual group (RHAG): its HABs, OCAB and 3x3 conv (None for resi_connection 'identity'), and the group-level routes:
    to_conv: the OCAB hands its result to the group conv as T rows;  conv_ln: (gamma, beta), gap_c of the LayerNorm the
    group conv emits from its epilogue, or None;  ocab16: the last tail, the OCAB projection and MLP carry FP16 rows;
    out16: the group conv writes its output as FP16 rows (hA)."""
    to_conv = ocab16 = out16 = False
    conv_ln = None

    def __init__(self, heads, habs, ocab, conv):
        self.heads, self.habs, self.ocab, self.conv = heads, habs, ocab, conv


class _Fwd:
    """The state of one forward, handed to every stage step: geometry, the workspace (a shallow copy: the steps swap the two
    LayerNorm-output buffers in it), the band, and what one step leaves for the next — t, the residual stream; gin, the
    current group's input; have_n, w["n"] already holds the next LayerNorm of t; have_n16, w["n16"] a compact copy of its
    first 16 channels; nblk, the number of GAP partial blocks in w["gap"]."""

    def __init__(self, eng, w, B, H, W, band, one_stream):
        self.B, self.H, self.W, self.N = B, H, W, H * W
        self.C, self.dt, self.ldc = eng.C, eng.dtype, _r8(eng.C)
        self.geo = dict(B=B, H=H, W=W, dtype=eng.dtype)
        self.w, self.band, self.one_stream = w, band, one_stream
        self.t = self.gin = w["tA"]
        self.have_n = self.have_n16 = False
        self.nblk = ops.layernorm_blocks()

    def ln(self, src, dst, gb, out_f32=False, gap_c=0):
        ops.layernorm(src, dst, gb[0], gb[1], B=self.B, npix=self.N, C_=self.C, ldy=(self.C if out_f32 else self.ldc),
                      out_f32=out_f32, dtype=self.dt, gap=(self.w["gap"] if gap_c else None), gap_c=gap_c)

    def pooled(self, src, ld, C_, dst, off=0, r0=None, r1=None, c0=0, c1=None):
        """dst[:, off:off + C_] = sums of src over this band's own rows (or rows [r0, r1)) x columns [c0, c1)."""
        bd, w = self.band, self.w
        ops.rect_sum(src, dst, w["rs_tmp"], w["rs_cnt"], B=self.B, W=self.W, ld=ld, C_=C_, r0=(bd.lo if r0 is None else r0),
                     r1=(bd.lo + bd.own if r1 is None else r1), c0=c0, c1=c1, out_off=off)

    def gstat(self, esc):
        """(local, global) ESC pool vectors as (B, 16) views, (B, 32) for pdim > 16: hat_esc_weights reads one block
        of that many floats per sample, whatever width the workspace gives the buffers (yw)."""
        gs = 32 if esc.pdim > 16 else 16
        return tuple(self.w[k].view(-1)[:self.B * gs].view(self.B, gs) for k in ("gstat_l", "gstat_g"))


class HATEngine(FrameBoundary, EngineBase):
    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], device, dtype: str = "bf16", options: Optional[Options] = None):
        """options: the switches (default: Options.from_env(), the environment's)."""
        if cfg.get("upsampler") != "pixelshuffle":
            raise NotImplementedError("only upsampler='pixelshuffle' is on the hot path (all shipped test YAMLs)")
        if cfg.get("resi_connection", "1conv") not in ("1conv", "identity"):
            raise ValueError(f"Unknown resi_connection: {cfg.get('resi_connection')}")   # hat_arch.py:547-548, :750-751
        self.cfg = cfg
        self.opt = Options.from_env() if options is None else options
        self.identity = cfg.get("resi_connection", "1conv") == "identity"
        if torch.device(device).type != "cuda":
            raise RuntimeError("HATEngine needs a GPU device: there is no CPU path")
        super().__init__(device, dtype, int(os.environ.get("HAT_WS_CACHE", "12")))
        self.C = cfg["embed_dim"]
        self.ws = cfg["window_size"]
        self.wse = self.ws + int(cfg["overlap_ratio"] * self.ws)
        self.scale = cfg["upscale"]
        self.fp16_fallbacks = 0
        self.u8_fused_calls = self.u8_planes_calls = 0   # 8-bit forwards that ended in hat_conv3x3_to_u8 / in hat_planes_to_u8
        self.yuv_fused_calls = self.yuv_planes_calls = 0   # YCbCr forwards that ended in hat_conv3x3_to_yuv / in hat_planes_to_yuv
        self.use_n16 = not self.opt.no_n16
        # FP16 residual rows between the fused HAB tails of a residual group (bf16 path, embed_dim 144; HAT_NO_T16=1: fp32 everywhere)
        self.t16 = not self.opt.no_t16 and self.dtype == ops.HAT_BF16 and self.C == 144
        # the guard of that stream (_T16Guard): the mode, what it has seen, and its state; no FP16 stream, no guard
        self.t16_guard = self.opt.t16_guard
        self.t16_fallbacks = self.t16_clipped_frames = 0   # switches to the fp32 stream; clipped frames that were already handed out
        self.t16_peak = 0.0                                # the magnitude the stream peaked at when it fell back
        self._guard = _T16Guard(self.dev) if self.t16 else None
        self._armed = False                                # this forward launches the guarded entries
        self._s1 = None
        ops._lib.load()
        # HATX (hatx_arch.py): the SGFN runs as fc1 -> hat_sgfn_gate -> fc2; odd window overlaps are padded with
        # ceil((wse - ws) / 2) (hatx_arch.py:303-305) and run on the generic attention kernel (key windows 25 and 13)
        self.hatx = cfg.get("variant", "hat") == "hatx"
        self.topk = float(cfg.get("kv_topk_ratio", 1.0)) if self.hatx else 1.0
        self.focus = bool(cfg.get("use_focus_bias", False)) if self.hatx else False
        # fused FFN kernel (hat_ffn) for the shapes it is instantiated for, else the unfused fc1 -> dw+gate -> fc2
        self.fuse_ffn = not self.hatx and ops.ffn_supported(self.C) and not self.opt.no_fused_ffn
        self._pack(state_dict)
        self._resolve()

    # ------------------------------------------------------------------------------------------
    def _lin(self, sd, wkey, bkey, scale=1.0):
        """Pack a pointwise layer for hat_linear when its shape is instantiated, else for hat_conv (ksize 1)."""
        w = sd[wkey]
        b = sd.get(bkey) if bkey else None
        o, i = w.shape[0], w.reshape(w.shape[0], -1).shape[1]

        pack = lambda wm, bias: ops.pack_pointwise(wm, bias, self.dtype, self.dev, scale=scale)
        w2 = w.reshape(o, -1)
        if w2.shape[1] == i and i > 512 and i % 16 == 0 and not ops.linear_supported(o, i, self.dtype):
            # K too wide for any tiling (HATX's SGFN fc2 at embed_dim 180: 720 -> 180; its fp32 rows do not fit a hat_conv tile):
            # two launches over the two halves of K, the second adding onto the first's fp32 result
            h1, h2 = pack(w2[:, :i // 2].contiguous(), b), pack(w2[:, i // 2:].contiguous(), None)
            h1.ksplit = h2
            return h1
        return pack(w, b)

    def _c3(self, sd, wkey, bkey):
        """Pack a CAB 3x3 conv for hat_conv3x3_small (weights resident in LDS) when instantiated, else for hat_conv."""
        w = sd[wkey]
        # squeeze conv (C -> C/cr, one n-tile): hat_conv's LDS-staged haloed tile beats gathering 9 neighbours per
        # k-step through L1 (0.18 vs 0.23 ms at 720p); expand conv (C/cr -> C, K = 72): the gathers are cheap, tap3 wins
        if w.shape[0] > 16 and ops.conv3x3_small_supported(w.shape[0], w.shape[1], self.dtype):
            return ops.pack_linear_weight(w, sd[bkey], self.dtype, self.dev)
        return ops.pack_conv_weight(w, sd[bkey], self.dtype, self.dev)

    def _esc(self, sd, core, plk_key, pdim, ksize):
        esc = _ESC(sd, core, plk_key, pdim, ksize, self.C, self.dtype, self.dev)
        esc.aggr = self._lin(sd, *esc.aggr_keys)
        esc.conv13 = ops.esc_conv13_supported(pdim, ksize, self.dtype) and not self.opt.no_esc13
        return esc

    def _run_lin(self, pw, x, out, **kw):
        h2 = getattr(pw, "ksplit", None)
        if h2 is not None:   # out = W[:, :K/2] x[:, :K/2] + b (+ r1), then out += W[:, K/2:] x[:, K/2:]   (fp32 output only)
            if kw.get("out_mode") != O_NHWC_F32 or kw.get("act", ACT_NONE) != ACT_NONE:
                raise NotImplementedError("a K-split linear accumulates through its fp32 output")
            (ops.linear if pw.frag else ops.conv)(pw, x, out, **kw)
            (ops.linear if h2.frag else ops.conv)(h2, x.reshape(-1)[pw.cin:], out, **dict(kw, r1=out, ldr1=kw["ldo"]))
            return
        (ops.linear if pw.frag else ops.conv)(pw, x, out, **kw)

    def _pack(self, sd):
        cfg, dev = self.cfg, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        P = lambda w, b=None, **kw: ops.pack_conv_weight(sd[w], None if b is None else sd[b], self.dtype, dev, **kw)
        vec = lambda k: sd[k].detach().to(**f32).contiguous()
        self.naf = self._pack_naf(sd) if cfg.get("naf") else None
        self.conv_first = P("conv_first.weight", "conv_first.bias")
        self.pe_norm = (vec("patch_embed.norm.weight"), vec("patch_embed.norm.bias")) if cfg.get("patch_norm", True) else None
        self.ape = vec("absolute_pos_embed").reshape(-1) if cfg.get("ape", False) else None   # (num_patches * C,)  :699-702
        self.layers = []
        for g, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
            habs = [self._pack_hab(sd, f"layers.{g}.residual_group.blocks.{i}") for i in range(depth)]
            ocab = self._pack_ocab(sd, f"layers.{g}.residual_group.overlap_attn", heads)
            self.layers.append(_Group(heads, habs, ocab, None if self.identity else P(f"layers.{g}.conv.weight", f"layers.{g}.conv.bias")))
        self.norm = (vec("norm.weight"), vec("norm.bias"))
        self.conv_after_body = None if self.identity else P("conv_after_body.weight", "conv_after_body.bias")
        self.conv_before_up = P("conv_before_upsample.0.weight", "conv_before_upsample.0.bias")
        self.ups = []
        s = self.scale
        if s & (s - 1) == 0:
            for i in range(int(math.log2(s))):
                self.ups.append((self._pack_ps(sd, f"upsample.{2 * i}", 2), 2))
        elif s == 3:
            self.ups.append((self._pack_ps(sd, "upsample.0", 3), 3))
        else:
            raise ValueError(f"scale {s} is not supported. Supported scales: 2^n and 3.")
        self.conv_last = P("conv_last.weight", "conv_last.bias")
        wl = sd["conv_last.weight"]
        self.conv_last_sweep = None   # row-sweep kernel (no LDS) for the 64 -> 3 conv at output resolution
        if ops.conv3x3_to_planes_supported(wl.shape[0], wl.shape[1], 16, self.dtype) and not self.opt.no_cab_sweep:
            self.conv_last_sweep = ops.pack_cab_squeeze(wl, sd["conv_last.bias"], dev) + (wl.shape[0],)
        # The folded ending (hat_upfold_*): the last PixelShuffle(2) conv and conv_last as one 5x5 conv on that stage's input, where
        # conv_last's row sweep is packed for three colours (so u8_fused says the same of both endings).  x4: the first stage is
        # unchanged; x2: the only stage.  x3, fp32 and other widths keep the two launches; _folded adds the per-shape width rule.
        self.upfold = None
        if self.ups and self.ups[-1][1] == 2 and self.conv_last_sweep is not None and not self.opt.no_upfold:   # (x1 has no stage)
            key = f"upsample.{2 * (len(self.ups) - 1)}"
            wu = sd[key + ".weight"]
            if ops.upfold_supported(wu.shape[1], wl.shape[0], 2, 16, self.dtype) and wl.shape[1] * 4 == wu.shape[0]:
                self.upfold = ops.pack_upfold(wu, sd[key + ".bias"], wl, sd["conv_last.bias"], dev)

    def _pack_naf(self, sd):
        """cfg["naf"] = {width, blocks}: the stem in front of the network, parameters under "naf." (the rest of sd is HATX's own
        surface).  Widths hat_naf_half is not built for and an in_chans other than 3 are refused here: there is no other path."""
        c, nb = int(self.cfg["naf"]["width"]), int(self.cfg["naf"]["blocks"])
        if c not in ops.NAF_WIDTHS:
            raise ValueError(f"naf_width {c} is not supported: hat_naf_half is built for {' and '.join(map(str, ops.NAF_WIDTHS))} channels")
        if self.cfg["in_chans"] != 3:
            raise ValueError(f"the NAF stem's head and tail convs are packed for in_chans 3, got {self.cfg['in_chans']}")
        P = lambda k: ops.pack_conv_weight(sd[f"naf.{k}.weight"], sd[f"naf.{k}.bias"], self.dtype, self.dev)
        return _Naf(c, P("head"), [ops.pack_naf_block(sd, f"naf.body.{i}", self.dtype, self.dev) for i in range(nb)], P("tail"))

    def _pack_hab(self, sd, p):
        """Packs one HAB.  Sets tail144_ok / tail180_ok; _resolve turns them into the tail route once the whole net is packed."""
        cfg, dt, dev, C, opt = self.cfg, self.dtype, self.dev, self.C, self.opt
        f32 = dict(dtype=torch.float32, device=dev)
        vec = lambda k: sd[k].detach().to(**f32).contiguous()
        hb = _Hab()
        hb.n1 = (vec(p + ".norm1.weight"), vec(p + ".norm1.bias"))
        hb.n2 = (vec(p + ".norm2.weight"), vec(p + ".norm2.bias"))
        hb.esc = self._esc(sd, p + ".esc_attn.core", p + ".esc_attn.plk_filter", cfg["esc_pdim"], cfg["esc_kernel"])
        hb.cab0 = self._c3(sd, p + ".conv_block.cab.0.weight", p + ".conv_block.cab.0.bias")
        hb.cab2 = self._c3(sd, p + ".conv_block.cab.2.weight", p + ".conv_block.cab.2.bias")
        hb.eca_w = vec(p + ".conv_block.cab.3.conv.weight").reshape(-1)
        w2raw = sd[p + ".conv_block.cab.2.weight"]
        # CAB expand conv + ECA folded into the aggregation (hat_cab_fold / hat_aggr_cab): squeeze width <= 8 only
        if hb.esc.aggr.frag and not hb.cab0.frag and ops.aggr_cab_supported(C, w2raw.shape[1], dt) and not opt.no_cab_fold:
            hb.fold = {"w2": w2raw.detach().to(**f32).contiguous(), "b2": vec(p + ".conv_block.cab.2.bias"),
                       "ba": vec(hb.esc.aggr_keys[1]), "w2f": ops.pack_cab_w2f(w2raw, dev)}
            # squeeze conv on the row-sweep kernel (no LDS operand traffic) where it is instantiated
            if ops.cab_squeeze_supported(C, w2raw.shape[1], 16, dt) and not opt.no_cab_sweep:
                hb.fold["sq"] = ops.pack_cab_squeeze(sd[p + ".conv_block.cab.0.weight"], sd[p + ".conv_block.cab.0.bias"], dev)
        if not self.fuse_ffn:
            hb.fc1 = self._lin(sd, p + ".mlp.fc1.weight", p + ".mlp.fc1.bias")
            hb.fc2 = self._lin(sd, p + ".mlp.fc2.weight", p + ".mlp.fc2.bias")
        hid2 = sd[p + ".mlp.dw.weight"].shape[0]     # (HATX: the first half of the SGFN's hidden width)
        hb.dw_w = sd[p + ".mlp.dw.weight"].detach().to(**f32).reshape(hid2, 9).t().contiguous()  # [9][2*hid]
        hb.dw_b = vec(p + ".mlp.dw.bias")
        hb.tail144_ok = hb.tail180_ok = False
        if not self.fuse_ffn:
            return hb
        fw = [sd[p + k] for k in (".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.dw.weight", ".mlp.dw.bias", ".mlp.fc2.weight", ".mlp.fc2.bias")]
        # hat_ffn2 (fp16 hidden tensor, depthwise conv on the packed-fp16 VALU) where it is built; HAT_FFN_V1=1 keeps the
        # first-generation kernel for A/B runs ... unless this block's weights could drive its FP16 hidden tensor past the FP16
        # range for SOME input (pack-time worst-case bound, ops.ffn_fp16_range_bound): then the bf16-hidden kernel stays
        fp16_ok = ops.ffn_fp16_range_bound(fw[0], fw[1], fw[2], fw[3], *hb.n2) < ops.FP16_SAFE
        if not fp16_ok:
            self.fp16_fallbacks += 1
        if ops.ffn2_supported(C, hid2 // 2, dt) and not opt.ffn_v1 and fp16_ok:
            hb.ffn = ops.pack_ffn2(*fw, dev)
        else:
            hb.ffn = ops.pack_ffn(*fw, dt, dev)
        hb.tail144_ok = (hb.fold is not None and hb.esc.pdim == 16 and ops.hab_tail_supported(hb.ffn, hb.esc.aggr, w2raw.shape[1], dt)
                         and not opt.no_hab_tail)
        # third-generation tail (activation-stationary fc1, weights shared through LDS): its own packing.  tail144_ok is the ONE
        # condition of "fused144" and means ffn3 is packed: hab_tail_supported admits only hat_ffn2's packing of hb.ffn here,
        # and ffn2_supported and tail3_supported are the same predicate at embed_dim 144
        if hb.tail144_ok:
            hb.ffn3 = ops.pack_ffn3(*fw, *hb.n2, dev)
        # embed_dim 180 (HAT / HAT-L): hat_hab_tail3 with the CAB's c2 as a map (their squeeze is 60 wide: no fold)
        if (hb.fold is None and C == 180 and fp16_ok and ops.tail3_supported(C, hid2 // 2, dt) and hb.esc.pdim == 16
                and hb.esc.aggr.frag and not opt.no_hab_tail):
            f3 = ops.pack_ffn3(*fw, *hb.n2, dev)
            if ops.hab_tail_supported(f3, hb.esc.aggr, w2raw.shape[1], dt):
                hb.ffn3, hb.tail180_ok = f3, True
                hb.bias256 = torch.zeros(256, **f32)
                hb.bias256[:C] = vec(hb.esc.aggr_keys[1])
        return hb

    def _pack_ocab(self, sd, p, heads):
        cfg, dt, dev, C = self.cfg, self.dtype, self.dev, self.C
        vec = lambda k: sd[k].detach().to(dtype=torch.float32, device=dev).contiguous()
        ws, wse = self.ws, self.wse
        M = ws + wse - 1
        shift = (ws - wse + 1 - (ws - 1)) * (M + 1)  # rotated index i' -> reference index rpi = i' + shift (may be < 0)
        rot = (torch.arange(M * M) + shift) % (M * M)  # negative-index wraparound of hat_arch.py:378
        d = C // heads
        qscale = cfg.get("qk_scale") or d ** -0.5
        # the tuned OCAB kernel of the embed_dim-144 models takes its queries in log2 units: fold log2(e) into the q
        # projection too (before the weights are rounded), not into the kernel (HAT_NO_ATTN_LOG2=1: the round-2 kernel)
        qlog2 = (ops.ocab_attention_log2_supported(C, heads, ws, wse, dt) and not (self.focus or self.topk < 1.0)
                 and not self.opt.no_attn_log2 and d % 2 == 0 and _r8(C) == C)
        if qlog2:
            qscale = qscale * ops.LOG2E
        table = sd[p + ".relative_position_bias_table"].detach().to(torch.float32).cpu()  # (M*M, heads)
        oc = _Ocab()
        oc.n1 = (vec(p + ".norm1.weight"), vec(p + ".norm1.bias"))
        oc.n2 = (vec(p + ".norm2.weight"), vec(p + ".norm2.bias"))
        oc.q = self._lin(sd, p + ".q_proj.weight", p + ".q_proj.bias", scale=qscale)   # q * scale (hat_arch.py:375) folded in
        oc.kv = self._lin(sd, p + ".kv_proj.weight", p + ".kv_proj.bias")
        oc.proj = self._lin(sd, p + ".proj.weight", p + ".proj.bias")
        oc.mlp0 = self._lin(sd, p + ".mlp.0.weight", p + ".mlp.0.bias")
        oc.mlp2 = self._lin(sd, p + ".mlp.2.weight", p + ".mlp.2.bias")
        # both MLP layers in one launch where hat_ocab_mlp is built (HAT_NO_OCAB_MLP=1: the two hat_linear launches)
        if ops.ocab_mlp_supported(C, sd[p + ".mlp.0.weight"].shape[0], dt) and _r8(C) == C and not self.opt.no_ocab_mlp:
            oc.mlpf = ops.pack_ocab_mlp(sd[p + ".mlp.0.weight"], sd[p + ".mlp.0.bias"], sd[p + ".mlp.2.weight"], sd[p + ".mlp.2.bias"], dev)
        oc.bias_rot = table[rot].t().contiguous().to(dev)  # [heads][M*M]
        oc.qlog2 = qlog2
        # q and kv projections in one launch (both read LayerNorm1's output) where hat_ocab_qkv is built and the OCAB has
        # no ESC on its key / value path (HAT_NO_OCAB_QKV=1: two hat_linear launches on two streams)
        if C == 144 and dt == ops.HAT_BF16 and not cfg.get("ocab_esc_enable", False) and not self.opt.no_ocab_qkv:
            oc.qkvf = ops.pack_ocab_qkv(sd[p + ".q_proj.weight"], sd.get(p + ".q_proj.bias"), sd[p + ".kv_proj.weight"],
                                        sd.get(p + ".kv_proj.bias"), qscale, dev)
        if cfg.get("ocab_esc_enable", False):
            oc.esc = self._esc(sd, p + ".esc_core", p + ".esc_plk", cfg["ocab_esc_pdim"], cfg["ocab_esc_kernel"])
        if self.focus:  # saliency head: 1x1 C -> C/4, GELU, 1x1 -> 1                     hatx_arch.py:357-361
            oc.fh0 = ops.pack_conv_weight(sd[p + ".focus_head.0.weight"], sd[p + ".focus_head.0.bias"], dt, dev)
            oc.fh2 = ops.pack_conv_weight(sd[p + ".focus_head.2.weight"], sd[p + ".focus_head.2.bias"], dt, dev)
        return oc

    def _pack_ps(self, sd, key, r):
        """Conv feeding nn.PixelShuffle(r) (hat_arch.py:598-602): output channel c*r^2 + i*r + j is stored
        as packed row (i*r + j)*Cps + c so one lane's 4 consecutive channels land in ONE output pixel."""
        w = sd[key + ".weight"]
        o = w.shape[0]
        cps = o // (r * r)
        n = torch.arange(o)
        perm = (n % cps) * (r * r) + n // cps  # packed row n' = ij*cps + c  <-  original channel c*r^2 + ij
        return ops.pack_conv_weight(w, sd[key + ".bias"], self.dtype, self.dev, out_perm=perm)

    def _resolve(self):
        """Every launch route that does not depend on the input shape, decided once for the packed network."""
        layers, dt, C = self.layers, self.dtype, self.C
        escs = [hb.esc for G in layers for hb in G.habs] + [G.ocab.esc for G in layers if G.ocab.esc is not None]
        wide = any(e.npad > 16 for e in escs)   # the 144 tail reads the ESC conv output as 16-channel rows
        for gi, G in enumerate(layers):
            oc = G.ocab
            for i, hb in enumerate(G.habs):
                nh = G.habs[i + 1] if i + 1 < len(G.habs) else None
                hb.next_ln = (nh.n1, nh.esc.pdim) if nh is not None else (oc.n1, oc.esc.pdim if oc.esc is not None else 0)
                # (the 144 tail is ruled out network-wide by any wide ESC, the 180 tail only by its consumer's: kept as found)
                if hb.fold is not None:
                    hb.tail = "fused144" if hb.tail144_ok and not wide else "aggr_cab"
                else:
                    hb.tail = "fused180" if hb.tail180_ok and hb.next_ln[1] <= 16 else "aggr"
            # the OCAB's last layer hands its result to the group's 3x3 conv as T rows
            G.to_conv = bool(G.conv is not None and dt == ops.HAT_BF16 and _r8(C) == C and oc.mlp2.frag and not self.opt.no_bf16_conv_in)
            cv = G.conv
            if cv is not None and dt == ops.HAT_BF16 and not self.opt.no_conv_ln and cv.n_slices == 1 and cv.nout == cv.nt * 16:
                if gi + 1 < len(layers):
                    nhs = layers[gi + 1].habs
                    nxt, gap_c = (nhs[0].n1, nhs[0].esc.pdim) if nhs else (None, 0)
                else:
                    nxt, gap_c = (self.norm, 0) if self.conv_after_body is not None else (None, 0)
                G.conv_ln = (nxt, gap_c) if nxt is not None and gap_c in (0, 4, 8, 12, 16) else None
        # the head in one launch (hat_head_fused) when the first block takes what it emits: the fused tail's prologue reads n, its
        # compact copy and hat_layernorm's GAP partials.  The absolute position embedding sits between the two LayerNorms: not fused.
        hb0 = layers[0].habs[0] if layers and layers[0].habs else None
        self.head_fused = bool(not self.opt.no_head_fused and hb0 is not None and hb0.tail == "fused144" and self.pe_norm is not None
                               and self.ape is None and ops.head_fused_supported(self.conv_first, C, hb0.esc.pdim, dt))
        self._plan_t16()
        # 8-bit output (forward_to_u8 / forward_u8): conv_last's row-sweep kernel converts in its epilogue when it is packed for
        # three output channels (the width condition, W % 16, is the one _upsample already checks per shape); otherwise
        # conv_last writes fp32 planes and hat_planes_to_u8 converts them
        self.u8_fused = self.conv_last_sweep is not None and self.conv_last_sweep[2] == 3
        # what every workspace is sized by
        hab0 = layers[0].habs[0] if layers and layers[0].habs else None
        self._hab0 = hab0
        self._yw = max([16] + [e.npad for e in escs])      # channels of the ESC conv output / floats per GAP partial block
        self._kpad = max([hab0.esc.kpad if hab0 else 0] + [G.ocab.esc.kpad for G in layers if G.ocab.esc is not None])

    def _plan_t16(self):
        """Where the residual stream is handed over as FP16 rows (bf16 path at embed_dim 144, HAT_NO_T16=1: nowhere; called again
        when the guard switches the stream to fp32).
        A hand-over is FP16 only when EVERY reader of that buffer takes FP16 rows: hat_hab_tail3 (t_in / t_out), the OCAB
        projection (hat_linear: r1 and its output, in place), hat_ocab_mlp (r1) and the group conv (hat_conv: r1 and its
        output, in place).  hat_layernorm, hat_add_f32, the unfused OCAB / conv-LN fallbacks and the embed_dim-180 tail read
        fp32.  Sets G.ocab16, G.out16 (group input of the next group, or the stream after the last group) and hb.out16: the
        three kinds of launch that STORE FP16 rows, and so the three the guard replaces by their guarded entries
        (guarded_launches): the tail of a block with out16, the projection of a group with ocab16, the conv of one with out16."""
        layers = self.layers
        for G in layers:
            G.ocab16 = G.out16 = False
            for hb in G.habs:
                hb.out16 = False
        if not self.t16:
            return
        tail16 = lambda hb: hb.tail == "fused144" and hb.ffn3.C == 144
        conv16 = lambda G: bool(G.conv is not None and not G.conv.frag and G.conv.ksize > 1 and G.conv.nt == 9
                                and G.conv.n_slices == 1 and G.conv.nout == 144)
        for G in layers:
            oc = G.ocab
            G.ocab16 = bool(G.habs and tail16(G.habs[-1]) and G.to_conv and oc.mlpf is not None and oc.proj.frag
                            and oc.proj.nt == 9 and getattr(oc.proj, "ksplit", None) is None and oc.esc is None)
            for i, hb in enumerate(G.habs):
                # the stream leaves as FP16 rows when its reader takes them: the next fused tail, or, after the last block,
                # the OCAB projection and MLP (43.7 -> 43.6 dB at 720p by emulation)
                hb.out16 = tail16(hb) and (G.ocab16 if i + 1 == len(G.habs) else tail16(G.habs[i + 1]))
        for gi, G in enumerate(layers):
            if not conv16(G) or G.conv_ln is None:   # (without the fused LayerNorm, hat_layernorm reads the output)
                continue
            if gi + 1 < len(layers):
                nG = layers[gi + 1]
                G.out16 = bool(nG.habs and tail16(nG.habs[0]) and conv16(nG))
            else:
                G.out16 = self.conv_after_body is not None     # (the stream itself is not read after the last group)

    def guarded_launches(self):
        """The launches that go through a *_guarded entry while the guard is on, in launch order: ("tail", group, block),
        ("proj", group), ("conv", group).  Exactly the FP16 stores of _plan_t16; none with t16_guard "off" or without the stream."""
        if not self.t16 or self.t16_guard == "off":
            return []
        out = []
        for gi, G in enumerate(self.layers):
            out += [("tail", gi, i) for i, hb in enumerate(G.habs) if hb.out16]
            out += [("proj", gi)] if G.ocab16 else []
            out += [("conv", gi)] if G.out16 else []
        return out

    # ------------------------------------------------------------------------------------------ the FP16-range guard
    @contextlib.contextmanager
    def guard_mode(self, mode: str):
        """The guard's mode for the forwards inside the block: callers that wait for every frame anyway take "sync", the plan
        recorder "off".  A fallback that happens inside outlives the block."""
        if mode not in T16_GUARD_MODES:
            raise ValueError(f"t16_guard is one of {', '.join(T16_GUARD_MODES)}, got {mode!r}")
        with self._lock:      # (not across the block: the forwards inside take the lock themselves)
            old, self.t16_guard = self.t16_guard, mode
        try:
            yield self
        finally:
            with self._lock:
                self.t16_guard = old

    @contextlib.contextmanager
    def head_route(self, fused: bool):
        """The head's route for the forwards inside the block: hat_head_fused where _resolve chose it (fused=True), or the three
        launches it equals bit for bit (the plan recorder: hat_head_fused is not in the plan format's function table)."""
        with self._lock:
            old, self.head_fused = self.head_fused, bool(fused and self.head_fused)
        try:
            yield self
        finally:
            with self._lock:
                self.head_fused = old

    def _sat(self, stores16: bool):
        """The slot a launch that stores FP16 rows reports to, or None: the unguarded entry."""
        return self._guard.slot if stores16 and self._armed else None

    def _guard_begin(self) -> bool:
        """Before the first launch of a forward (under the lock, not while a graph is being captured): look at the word of
        earlier forwards if their event has passed — never waiting — then arm this one and zero the slot."""
        g = self._guard
        if g is None:
            return False
        if g.pending and g.event.query():
            self._guard_look()
        self._armed = self.t16 and self.t16_guard != "off"
        if self._armed and not g.pending:
            g.slot.zero_()
        return self._armed

    def _guard_look(self):
        """The pending word: clean, or the frames it covers were handed out clipped — count them, warn once, leave the FP16 stream."""
        g = self._guard
        word, n, g.pending = g.word(), g.pending, 0
        if word and self.t16:
            self.t16_clipped_frames += n
            self._t16_fall_back(word)
            warnings.warn(f"the FP16 residual stream left the FP16 range (peaked at {self.t16_peak:.4g}, limit 65504): {n} frame"
                          f"{'s' if n != 1 else ''} already returned {'were' if n != 1 else 'was'} clipped; this engine carries "
                          f"the stream in fp32 from now on (t16_guard='sync' re-runs such a frame before it is returned)", RuntimeWarning, stacklevel=3)

    def _t16_fall_back(self, word: int):
        """Switch to the fp32 stream for the life of the engine: what HAT_NO_T16=1 runs.  Workspaces of the old plan are dropped
        (a HIP graph captured on one keeps it alive and is dropped by its owner, whose cache key holds t16)."""
        self.t16, self._armed = False, False
        self.t16_fallbacks += 1
        self.t16_peak = ops.read_sat(word)
        self._plan_t16()
        self._ws_cache.clear()

    def _guard_end(self, defer: bool = False) -> bool:
        """Behind the last launch of an armed forward (not while capturing: a graph's owner calls it behind the replay): record
        the copy of the slot to the host word and the event behind it (defer=True: "defer" whatever the mode).  "sync": wait for it; True when the stream clipped and the engine has fallen back —
        the caller runs the frame again.  "defer": leave the word to the next forward or to resolve_t16_guard."""
        g = self._guard
        if g is None or not self._armed:
            return False
        self._armed = False
        g.host.copy_(g.slot, non_blocking=True)
        g.event.record()
        if defer or self.t16_guard != "sync":
            g.pending += 1
            return False
        g.event.synchronize()
        word, earlier, g.pending = g.word(), g.pending, 0
        if not word:
            return False
        self.t16_clipped_frames += earlier   # (forwards deferred before this one share the word: counted as handed out clipped)
        self._t16_fall_back(word)
        return True

    def resolve_t16_guard(self) -> bool:
        """Wait for the forwards handed out so far and look at their word.  True: they stayed in the FP16 range (or there is no
        FP16 stream).  False: the engine is, or has just gone, on the fp32 stream; t16_clipped_frames, t16_fallbacks and
        t16_peak say what happened."""
        with self._lock:
            g = self._guard
            if g is not None and g.pending:
                g.event.synchronize()
                self._guard_look()
            return self.t16_fallbacks == 0

    # ------------------------------------------------------------------------------------------
    def _alloc_workspace(self, B, H, W, tag):
        """The buffers of one (B, H, W) input; a row band's (tag, EngineBase._workspace) also holds its pooled sums."""
        C, dev, T, hab0, yw = self.C, self.dev, self.tdt, self._hab0, self._yw
        N = H * W
        mid = hab0.cab0.nout if hab0 is not None else 8
        hid2 = 2 * int(C * self.cfg["mlp_ratio"])  # fc1 width of GatedDconvFFN (hat_arch.py:99-100)
        z = lambda *shape, dtype=T: torch.zeros(*shape, dtype=dtype, device=dev)
        f = torch.float32
        w = {
            "f0": z(B, N, C, dtype=f), "tA": z(B, N, C, dtype=f), "tB": z(B, N, C, dtype=f), "tC": z(B, N, C, dtype=f),
            # the residual stream as FP16 rows: hA = a group's input (written by the previous group conv), hB / hC = between its
            # fused tails and through its OCAB (see _plan_t16)
            "hA": (z(B, N, C, dtype=torch.float16) if self.t16 else None),
            "hB": (z(B, N, C, dtype=torch.float16) if self.t16 else None), "hC": (z(B, N, C, dtype=torch.float16) if self.t16 else None),
            "n": z(B, N, _r8(C)), "n2b": z(B, N, _r8(C)), "c1": z(B, N, _r8(mid)), "c2": z(B, N, _r8(C)), "m2": z(B, N, ops.ffn_m_ld(C)),
            "y16": z(B, N, yw), "n16": z(B, N, 16), "u": z(B, N, _r8(max(hid2, 2 * C))), "g": z(B, N, _r8(max(hid2 // 2, 2 * C))),
            "q": z(B, N, _r8(C)), "kv": z(B, N, _r8(2 * C)), "ao": z(B, N, _r8(C)),
            "fb": z(B, N, 64),
            "gap": z(B, max(ops.layernorm_blocks(), -(-H // 4) * -(-W // 16)), yw, dtype=f),
            "scale": z(B, 256, dtype=f), "eca_tmp": z(B, 32, 256, dtype=f),
        }
        if any(G.ocab.qkvf is not None for G in self.layers):
            w["qkv"] = z(B, N, 432)      # [q | k | v] rows of the fused projection
        w["weff"] = z(B, yw, max(self._kpad, 64))
        if any(G.ocab.esc is not None for G in self.layers):
            w["yesc"] = z(B, N, _r8(C))
        if self.focus:
            w["fh"], w["sal"] = z(B, N, _r8(C // 4)), z(B, N, 8, dtype=f)   # (the saliency map stays fp32: the keys are ranked on it)
        if self.focus or self.topk < 1.0:
            w["kb"] = z(B, (H // self.ws) * (W // self.ws), -(-(self.wse * self.wse) // 16) * 16, dtype=f)   # rows of whole key tiles
        if hab0 is not None:
            cab2 = hab0.cab2
            tiles = ops.conv3x3_small_groups(cab2, B, H, W, self.dtype) if cab2.frag else ops.conv_tiles(cab2, H, W, self.dtype)
            w["tiles"] = tiles
            w["colsum"] = z(B, tiles, cab2.npad, dtype=f)
        if hab0 is not None and hab0.fold is not None:
            cab0 = hab0.cab0
            w["sweep"] = "sq" in hab0.fold and W % 16 == 0 and cab0.npad == 16
            w["tiles1"] = ops.cab_squeeze_units(H, W) if w["sweep"] else ops.conv_tiles(cab0, H, W, self.dtype)
            w["colsum1"] = z(B, w["tiles1"], cab0.npad, dtype=f)
            w["wf"] = z(B, hab0.esc.aggr.nt * 3 * 512)
            w["bias_b"] = z(B, hab0.esc.aggr.npad, dtype=f)
        if tag is not None:   # pooled sums of this band's own rows (local) and of the whole frame (global): SURVEY §8 f4
            w["gstat_l"], w["gstat_g"] = z(B, yw, dtype=f), z(B, yw, dtype=f)
            w["cstat_l"], w["cstat_g"] = z(B, 72, dtype=f), z(B, 72, dtype=f)
            w["estat_l"], w["estat_g"] = z(B, 256, dtype=f), z(B, 256, dtype=f)
            w["rs_tmp"], w["rs_cnt"] = z(B, 64, 256, dtype=f), torch.zeros(B, dtype=torch.int32, device=dev)
        if self.naf is not None:   # the stem's two fp32 streams, two gated maps, pool partials, per-sample fold and result
            c = self.naf.c
            w["naf_sA"], w["naf_sB"], w["naf_gA"], w["naf_gB"] = z(B, N, c, dtype=f), z(B, N, c, dtype=f), z(B, N, c), z(B, N, c)
            w["naf_part"], w["naf_wf"], w["naf_bf"] = z(B, ops.naf_tiles(H, W), c, dtype=f), z(B, c * c), z(B, c, dtype=f)
            w["x_naf"] = z(B, self.cfg["in_chans"], H, W, dtype=f)
        h, wd = H, W
        w["ups"] = []
        for i, (_, r) in enumerate(self.ups):
            h, wd = h * r, wd * r
            # (the folded ending writes no shuffled map of its last stage)
            w["ups"].append(None if i + 1 == len(self.ups) and self._folded(W) else z(B, h * wd, 64))
        return w

    def _folded(self, W: int) -> bool:
        """Whether the forward of a W-wide input ends in hat_upfold_* (packed, and the last stage's input width is one the kernel
        takes): the ONE condition of _upsample's plain and sink branches and of the workspace."""
        if self.upfold is None:
            return False
        for _, r in self.ups[:-1]:
            W *= r
        return ops.upfold_supported(64, 3, 2, W, self.dtype)

    # ------------------------------------------------------------------------------------------
    def _esc_w(self, esc: _ESC, w, B, H, W, nblk, gap=None):
        """The per-sample 13x13 weights of the ESC conv (static filter + dynamic depthwise kernel) -> w['weff'].
        gap: one block of frame-wide sums over H * W pixels (band-sharded frames) instead of w['gap']'s nblk partial blocks."""
        ops.esc_weights(w["gap"] if gap is None else gap, nblk, H * W, esc.w1, esc.b1, esc.w2, esc.b2, esc.plk, w["weff"], B=B,
                        pdim=esc.pdim, ksize=esc.ksize, kpad=esc.kpad, dtype=self.dtype)

    def _esc_conv(self, esc: _ESC, w, n, B, H, W, n16=None):
        """n16: a compact (B,N,16) copy of n's first 16 channels when the producer wrote one (the fused HAB tail does)."""
        if esc.conv13:
            src, ldx = (n16, 16) if n16 is not None else (n, _r8(self.C))
            ops.esc_conv13(src, w["weff"], w["y16"], B=B, H=H, W=W, ldx=ldx, kpad=esc.kpad, dtype=self.dtype)
            return
        pw = ops.PackedConv(w["weff"], esc.zero_bias, esc.ksize, esc.pdim, esc.kpad, 1, esc.npad // 16, esc.pdim,
                            w_bstride=esc.npad * esc.kpad)
        ops.conv(pw, n, w["y16"], B=B, H=H, W=W, dtype=self.dtype, ldx=_r8(self.C), ldo=w["y16"].shape[2], n_store=_r4(esc.pdim))

    def _esc_lk(self, esc: _ESC, w, n, B, H, W, nblk):
        """ESC large-kernel + dynamic depthwise conv on the first pdim channels of `n` -> w['y16']."""
        self._esc_w(esc, w, B, H, W, nblk)
        self._esc_conv(esc, w, n, B, H, W)

    @staticmethod
    def _hab_halo(esc: _ESC) -> int:
        """Ghost rows a HAB reads beyond the band's own ones: LayerNorm1's output three rows (the two CAB convs under the FFN's
        depthwise 3x3), its first pdim channels ksize // 2 + 1 rows (the ESC conv under the same row)."""
        return max(3, esc.ksize // 2 + 1)

    def _ocab_halo(self, oc: _Ocab) -> int:
        """Ghost rows an OCAB reads: its key windows reach pad = ceil((wse - ws) / 2) rows beyond the query window (HATX's
        ceil padding, hatx_arch.py:315-321: pad above, pad - 1 below); with OCAB-ESC the keys are ESC(LN(x)), whose conv reads
        ksize // 2 rows further."""
        pad = (self.wse - self.ws + 1) // 2
        return pad + (oc.esc.ksize // 2 if oc.esc is not None else 0)

    def band_halo(self) -> int:
        """The deepest ghost-row refresh the band-sharded forward of this network requests (band_parallel.make_bands checks
        the band geometry against it): the largest of the HAB and OCAB refreshes and the 8 rows before the network's last
        convs.  HAT-S / HAT: 8; hatx_live_x2 shapes (ESC 15, OCAB-ESC 17, 13x13 key windows): 11; the live HATX config: 13."""
        d = 8
        for G in self.layers:
            d = max([d, self._ocab_halo(G.ocab)] + [self._hab_halo(hb.esc) for hb in G.habs])
        return d

    def _side_stream(self, f: _Fwd):
        """The stream the short independent chains go to: the current one for a band or with one_stream."""
        if f.band is not None or f.one_stream:
            return torch.cuda.current_stream(self.dev)
        if self._s1 is None:
            self._s1 = torch.cuda.Stream(device=self.dev)
        return self._s1

    def _check_input(self, x):
        """The shapes every forward refuses (_forward_gen calls it; an ensemble calls it before it allocates or launches)."""
        if x.dim() != 4 or x.shape[1] != self.cfg["in_chans"]:
            raise RuntimeError(f"expected (B,{self.cfg['in_chans']},H,W), got {tuple(x.shape)}")
        if x.shape[2] % self.ws or x.shape[3] % self.ws:  # the reference raises from calculate_mask's view (hat_arch.py:815), SURVEY F4
            raise RuntimeError(f"input size ({x.shape[2]},{x.shape[3]}) is not a multiple of window_size {self.ws}")

    def ocab_only(self, t: torch.Tensor, group: int, H: int, W: int) -> torch.Tensor:
        """Run only the OCAB of residual group `group` on tokens t (B, H*W, C) fp32 -> (B, H*W, C) fp32 (used by the tests)."""
        x = torch.zeros(t.shape[0], self.cfg["in_chans"], H, W, device=self.dev)
        with self._lock, torch.cuda.device(self.dev):
            return self._forward(x, only_ocab=(t.to(self.dev, torch.float32).contiguous(), group))

    def _forward(self, x: torch.Tensor, only_ocab=None, one_stream=None, sink=None) -> torch.Tensor:
        """one_stream: overrides HAT_ONE_STREAM for this call (plan export records the one-stream order).
        The guard brackets the launches: zero the slot, launch (guarded entries where FP16 rows are stored), copy the slot to
        the host word, record the event.  While a HIP graph is captured only the launches and the copy are recorded; the
        graph's owner zeroes before a replay and records behind it (archs/hat_arch.py)."""
        capturing = self._guard is not None and torch.cuda.is_current_stream_capturing()
        if capturing:
            self._armed = self.t16 and self.t16_guard != "off"
        else:
            self._guard_begin()
        y = self._launches(x, only_ocab=only_ocab, one_stream=one_stream, sink=sink)
        if self._armed:
            if capturing:
                self._guard.host.copy_(self._guard.slot, non_blocking=True)
                self._armed = False
            elif self._guard_end():   # "sync" and the stream clipped: the same frame on the fp32 stream
                y = self._launches(x, only_ocab=only_ocab, one_stream=one_stream, sink=sink)
        return y

    def _launches(self, x: torch.Tensor, only_ocab=None, one_stream=None, sink=None) -> torch.Tensor:
        gen = self._forward_gen(x, only_ocab=only_ocab, one_stream=one_stream, sink=sink)
        try:
            req = next(gen)
        except StopIteration as done:
            return done.value
        raise RuntimeError(f"the unsharded forward must not reach an exchange point (got {req[0]!r})")

    def _forward_gen(self, x: torch.Tensor, only_ocab=None, band=None, one_stream=None, sink=None):
        """The forward as a generator.  Unsharded (band=None) it never yields and returns the output.  For one ROW BAND of a
        sharded frame (band: tile_parallel.Band, x = the band's rows + ghost rows of the LR frame) it yields at
        every point where bands must exchange: ("halo", [(tensor, depth) ...]) — refresh `depth` ghost rows above and below
        from the neighbours that own them — and ("reduce", local, glob, n) — glob[:, :n] = sum over bands of local[:, :n] (the
        global average pools of ECA, hat_arch.py:69-73, and of the ESC dynamic kernel, esc_arch.py:96,121) — and returns the
        band's output rows (ghost rows included; the driver keeps the owned ones).
        sink (a _Sink; the unsharded forward only): the forward fills and returns sink.out, bytes, instead of fp32 planes."""
        self._check_input(x)
        if band is not None and self.naf is not None:
            raise NotImplementedError("a row band of a HybridHATNAF frame is not implemented: the stem's SCA pool needs one more "
                                      "reduce exchange and two more halo rows per NAF block")
        B, _, H, W = x.shape
        x = x.to(torch.float32).contiguous()
        w = dict(self._workspace(B, H, W, tag=(None if band is None else ("band", band.idx, band.n))))
        if band is not None and band.e1 - band.e0 != H:
            raise RuntimeError(f"band {band.idx} holds frame rows [{band.e0}, {band.e1}) but the input has {H} rows")
        f = _Fwd(self, w, B, H, W, band, self.opt.one_stream if one_stream is None else one_stream)
        if only_ocab is not None:   # test hook: one OCAB on a given residual stream (block-level parity against reference goldens)
            t_in, gidx = only_ocab
            w["tB"].copy_(t_in.reshape(B, H * W, self.C))
            f.t = w["tB"]
            return (yield from self._ocab(f, self.layers[gidx], as_conv_input=False)).clone()
        if sink is None:
            y = torch.empty(B, self.cfg["in_chans"], H * self.scale, W * self.scale, dtype=torch.float32, device=self.dev)
        elif band is not None:
            raise RuntimeError(sink.band_refusal)
        else:
            y = sink.out
        if self.naf is not None:
            x = self._naf_stem(f, x)
        self._head(f, x)
        for G in self.layers:
            for hb in G.habs:   # HAB                                                            :217-238
                yield from self._hab_prologue(f, hb)
                getattr(self, "_tail_" + hb.tail)(f, hb)
            tout = yield from self._ocab(f, G, as_conv_input=G.to_conv)
            yield from self._group_end(f, G, tout)
        yield from self._body_end(f)
        self._upsample(f, y, sink)
        return y

    # ------------------------------------------------------------------------------------------ stage steps
    def _naf_stem(self, f: _Fwd, x):
        """x + tail(body(head(x))) -> w["x_naf"], fp32 planes as _head reads them           hybrid_hat_naf_arch.py:77-82, :130-131
        head: hat_conv 3 -> c into the fp32 stream.  Per block: half (pw1, dw, gate; pool partials), hat_naf_fold (SCA into pw2),
        half (+ beta pw2 as its form (b); ffn1, ffn_dw, gate).  The block's last 1x1, gamma * ffn2, is the form (b) of the NEXT
        half; after the last block one projection-only launch.  The stream and the gated map alternate between two buffers
        each: a half reads its neighbours' halo pixels of both while it writes."""
        st, w, c = self.naf, f.w, self.naf.c
        kw = dict(B=f.B, H=f.H, W=f.W, C_=c, dtype=f.dt)
        s_in, s_out, g_in, g_out = w["naf_sA"], w["naf_sB"], w["naf_gA"], w["naf_gB"]
        ops.conv(st.head, x, s_in, **f.geo, ldx=0, ldo=c, x_mode=X_NCHW_F32_MEAN, out_mode=O_NHWC_F32)
        fold = None   # (wf, bf) of the previous block's gamma * ffn2
        for blk in st.blocks:
            if fold is None:
                ops.naf_half(s_in, g_out, blk.w1, blk.b1, blk.dww, blk.dwb, partials=w["naf_part"], **kw)
            else:
                ops.naf_half(s_in, g_out, blk.w1, blk.b1, blk.dww, blk.dwb, gprev=g_in, wf=fold[0], bf=fold[1], r_out=s_out,
                             partials=w["naf_part"], **kw)
                s_in, s_out = s_out, s_in
            g_in, g_out = g_out, g_in
            ops.naf_fold(w["naf_part"], blk, w["naf_wf"], w["naf_bf"], **kw)
            ops.naf_half(s_in, g_out, blk.w1f, blk.b1f, blk.dwwf, blk.dwbf, gprev=g_in, wf=w["naf_wf"], wf_bstride=c * c,
                         bf=w["naf_bf"], bf_bstride=c, r_out=s_out, **kw)
            s_in, s_out = s_out, s_in
            g_in, g_out = g_out, g_in
            fold = (blk.wf2, blk.bf2)
        if fold is not None:
            ops.naf_half(s_in, None, None, None, None, None, gprev=g_in, wf=fold[0], bf=fold[1], r_out=s_out, **kw)
            s_in = s_out
        ops.conv(st.tail, s_in, w["x_naf"], **f.geo, ldx=c, ldo=0, x_mode=X_NHWC_F32, out_mode=O_NCHW_F32)
        ops.add_f32(w["x_naf"], x, w["x_naf"], B=f.B, n=x.shape[1] * f.N)
        return w["x_naf"]

    def _head(self, f: _Fwd, x):
        """(x - mean) * img_range ; conv_first ; patch_embed LN ; + absolute_pos_embed     :836-838, :849-853"""
        w, tA, C = f.w, f.w["tA"], self.C
        r = float(self.cfg.get("img_range", 1.0))
        if self.head_fused:   # ... and the first block's norm1 with its compact copy and GAP partials: one launch
            hb0 = self._hab0
            ops.head_fused(self.conv_first, x, w["f0"], tA, w["n"], self.pe_norm, hb0.n1, B=f.B, H=f.H, W=f.W, ldn=f.ldc, dtype=f.dt,
                           in_scale=r, mean=self._mean(), n16=(w["n16"] if self.use_n16 else None), gap=w["gap"], gap_c=hb0.esc.pdim)
            f.have_n, f.have_n16, f.nblk = True, self.use_n16, ops.layernorm_blocks()
            return
        ops.conv(self.conv_first, x, w["f0"], **f.geo, ldx=0, ldo=C, x_mode=X_NCHW_F32_MEAN, out_mode=O_NHWC_F32,
                 in_scale=r, mean=self._mean())
        if self.pe_norm is not None:
            f.ln(w["f0"], tA, self.pe_norm, out_f32=True)
        else:
            tA.copy_(w["f0"])        # device-to-device copy on the current stream
        if self.ape is not None:   # (1, num_patches, C); a band adds ITS rows [e0, e1) of the frame's position table
            npix, off = (f.band.Hfull * f.W, f.band.e0 * f.W * C) if f.band is not None else (f.N, 0)
            if self.ape.numel() != npix * C:
                raise RuntimeError(f"absolute_pos_embed holds {self.ape.numel() // C} positions but the "
                                   f"{'frame' if f.band is not None else 'input'} has {npix} pixels (ape=True fixes the input "
                                   f"size to img_size, hat_arch.py:699-702)")
            ops.add_f32(tA, self.ape[off:off + f.N * C], tA, B=f.B, n=f.N * C, c_bstride=0)

    def _mean(self):
        return RGB_MEAN if self.cfg["in_chans"] == 3 else (0.0,) * 4

    def _hab_prologue(self, f: _Fwd, hb: _Hab):
        """LayerNorm1 (unless its producer emitted it), then the ESC branch and the CAB up to what the tail reads."""
        w, esc, bd = f.w, hb.esc, f.band
        if bd is not None and not f.have_n:   # (LayerNorm1 is recomputed on the ghost rows from the refreshed stream)
            yield ("halo", [(f.t, self._hab_halo(esc))])
        if not f.have_n:
            f.ln(f.t, w["n"], hb.n1, gap_c=esc.pdim)
            f.nblk, f.have_n16 = ops.layernorm_blocks(), False
        elif bd is not None:
            # what this block reads beyond the band's own rows: t one row (depthwise 3x3 of the FFN), LayerNorm1's
            # output three rows (the two CAB convs under it) and its first pdim channels ksize / 2 + 1 = seven rows
            # (13x13 conv under the FFN's halo row)
            er = esc.ksize // 2 + 1
            yield ("halo", [(f.t, 1)] + ([(w["n"], 3), (w["n16"], er)] if f.have_n16 else [(w["n"], self._hab_halo(esc))]))
        gst = None
        if bd is not None:   # the ESC pool (esc_arch.py:96,121) over the whole FRAME: this band's share, then the sum
            gst = f.gstat(esc)   # (summed over the bands together with the CAB pool: ONE reduce per HAB)
            if f.have_n16:
                f.pooled(w["n16"], 16, esc.pdim, gst[0])
            else:
                f.pooled(w["n"], f.ldc, esc.pdim, gst[0])
        if hb.fold is not None:
            yield from self._prologue_fold(f, hb, gst)
        else:
            yield from self._prologue_plain(f, hb, gst)

    def _squeeze_chain(self, f: _Fwd, hb: _Hab):
        """CAB squeeze conv -> c1 (+ its column sums), then hat_cab_fold (unsharded: a band folds after its reduce)."""
        w, fo = f.w, hb.fold
        if w["sweep"]:
            ops.cab_squeeze(w["n"], fo["sq"][0], fo["sq"][1], w["c1"], w["colsum1"], B=f.B, H=f.H, W=f.W, C_=self.C, ldx=f.ldc, dtype=f.dt)
        else:
            ops.conv(hb.cab0, w["n"], w["c1"], **f.geo, ldx=f.ldc, ldo=8, act=ACT_GELU, n_store=8, colsum=w["colsum1"])
        if f.band is None:
            ops.cab_fold(w["c1"], w["colsum1"], w["tiles1"], hb.cab0.npad, fo["w2"], fo["b2"], hb.eca_w, hb.eca_w.numel(),
                         fo["ba"], float(self.cfg["conv_scale"]), w["scale"], w["wf"], w["bias_b"], w["eca_tmp"], B=f.B, H=f.H,
                         W=f.W, C_=self.C, mid=hb.cab0.nout, dtype=f.dt, w2f=fo["w2f"])

    def _prologue_fold(self, f: _Fwd, hb: _Hab, gst):
        """c2 = conv3x3(c1) never exists: its ECA pooling follows from the sums of c1 (hat_cab_fold) and the scaled expand conv
        is three more k-steps of the aggregation GEMM (hat_aggr_cab).
        The two tiny per-sample kernels (one workgroup each, latency-bound) run on a side stream next to the convs they do not
        depend on: esc_weights beside the CAB squeeze conv, cab_fold beside the 13x13 conv.  The critical chain — ESC weight
        kernel -> 13x13 conv -> tail — stays on ONE stream: every hop between streams costs an event wait of ~12 us on this
        runtime (kernel trace: 2 hops per block = 0.9 ms per frame when the 13x13 conv sat on the side stream).  The CAB
        squeeze conv and its fold are shorter and go to the side stream (HAT_ESC_SIDE=1: the round-2 arrangement, for A/B)."""
        w, esc, B, H, W = f.w, hb.esc, f.B, f.H, f.W
        n16 = w["n16"] if f.have_n16 else None
        s0 = torch.cuda.current_stream(self.dev)
        s1 = self._side_stream(f)
        if f.band is not None:
            yield from self._fold_band(f, hb, gst)
            self._esc_w(esc, w, B, f.band.Hfull, W, 1, gap=gst[1])
            self._esc_conv(esc, w, w["n"], B, H, W, n16=n16)
        elif self.opt.esc_side:
            self._esc_w(esc, w, B, H, W, f.nblk)
            s1.wait_stream(s0)                              # n and the 13x13 weights are ready
            with torch.cuda.stream(s1):                     # chain 2: 13x13 conv
                self._esc_conv(esc, w, w["n"], B, H, W, n16=n16)
            self._squeeze_chain(f, hb)
        else:
            s1.wait_stream(s0)                              # n is ready
            with torch.cuda.stream(s1):
                self._squeeze_chain(f, hb)
            self._esc_w(esc, w, B, H, W, f.nblk)
            self._esc_conv(esc, w, w["n"], B, H, W, n16=n16)
        s0.wait_stream(s1)                                  # both chains are done

    def _fold_band(self, f: _Fwd, hb: _Hab, gst):
        """The band-sharded fold: the sums hat_cab_fold takes from c1 (hat_arch.py:73 via the linearity of the expand conv) are
        this band's share of [total | first row | last row | first column | last column | 4 corners], summed over the bands."""
        w, bd, W, fo = f.w, f.band, f.W, hb.fold
        self._squeeze_chain(f, hb)
        st, c1, lo, own = w["cstat_l"], w["c1"], bd.lo, bd.own
        f.pooled(c1, 8, 8, st, 0)
        f.pooled(c1, 8, 8, st, 24, c0=0, c1=1)
        f.pooled(c1, 8, 8, st, 32, c0=W - 1, c1=W)
        if bd.r0 == 0:
            f.pooled(c1, 8, 8, st, 8, r0=lo, r1=lo + 1)
            f.pooled(c1, 8, 8, st, 40, r0=lo, r1=lo + 1, c0=0, c1=1)
            f.pooled(c1, 8, 8, st, 48, r0=lo, r1=lo + 1, c0=W - 1, c1=W)
        if bd.r1 == bd.Hfull:
            f.pooled(c1, 8, 8, st, 16, r0=lo + own - 1, r1=lo + own)
            f.pooled(c1, 8, 8, st, 56, r0=lo + own - 1, r1=lo + own, c0=0, c1=1)
            f.pooled(c1, 8, 8, st, 64, r0=lo + own - 1, r1=lo + own, c0=W - 1, c1=W)
        yield ("reduce", [(gst[0], gst[1], hb.esc.pdim), (st, w["cstat_g"], 72)])
        ops.cab_fold(None, None, 1, hb.cab0.npad, fo["w2"], fo["b2"], hb.eca_w, hb.eca_w.numel(), fo["ba"],
                     float(self.cfg["conv_scale"]), w["scale"], w["wf"], w["bias_b"], None, B=f.B, H=bd.Hfull, W=W, C_=self.C,
                     mid=hb.cab0.nout, dtype=f.dt, stats=w["cstat_g"], w2f=fo["w2f"])

    def _prologue_plain(self, f: _Fwd, hb: _Hab, gst):
        """CAB squeeze and expand convs (c2), the ECA scale of c2, and the ESC conv."""
        w, esc, bd, B, H, W, C, ldc = f.w, hb.esc, f.band, f.B, f.H, f.W, self.C, f.ldc
        mid = hb.cab0.nout
        c3 = ops.conv3x3_small if hb.cab0.frag else ops.conv
        c3(hb.cab0, w["n"], w["c1"], **f.geo, ldx=ldc, ldo=_r8(mid), act=ACT_GELU, n_store=_r4(mid))
        c3 = ops.conv3x3_small if hb.cab2.frag else ops.conv
        c3(hb.cab2, w["c1"], w["c2"], **f.geo, ldx=_r8(mid), ldo=ldc, colsum=w["colsum"])
        if bd is None:
            ops.eca_scale(w["colsum"], w["tiles"], hb.cab2.npad, f.N, hb.eca_w, hb.eca_w.numel(),
                          float(self.cfg["conv_scale"]), w["eca_tmp"], w["scale"], B=B, C_=C)
            self._esc_lk(esc, w, w["n"], B, H, W, f.nblk)
            return
        # ECA pool of c2 (hat_arch.py:73) over the whole frame: this band's rows, then the sum over the bands (rows of npad
        # floats, like the per-tile column sums: hat_eca_scale writes `scale` with that stride and the aggregation reads it so)
        npd = hb.cab2.npad
        el, eg = (w[k].view(-1)[:B * npd].view(B, npd) for k in ("estat_l", "estat_g"))
        f.pooled(w["c2"], ldc, C, el)
        yield ("reduce", [(gst[0], gst[1], esc.pdim), (el, eg, _r4(C))])
        ops.eca_scale(eg, 1, npd, bd.Hfull * W, hb.eca_w, hb.eca_w.numel(), float(self.cfg["conv_scale"]), w["eca_tmp"],
                      w["scale"], B=B, C_=C)
        self._esc_w(esc, w, B, bd.Hfull, W, 1, gap=gst[1])
        self._esc_conv(esc, w, w["n"], B, H, W)

    def _tail_fused144(self, f: _Fwd, hb: _Hab):
        """Aggregation + folded CAB + residuals + the whole FFN in ONE launch: tB never exists in HBM (also the faster choice on
        small frames: 64x64 HAT-S 3.97 vs 6.19 ms per forward)."""
        w, t = f.w, f.t
        if hb.out16:
            tout = w["hB"] if t is not w["hB"] else w["hC"]
        else:
            tout = w["tB"] if t is not w["tB"] else w["tC"]
        nxt, gap_c = hb.next_ln
        ops.hab_tail(hb.ffn3, hb.esc.aggr, t, tout, hb.n2[0], hb.n2[1], n=w["n"], ldn_in=f.ldc,
                     y16=w["y16"], c1=w["c1"], wf=w["wf"], bias_b=w["bias_b"], B=f.B, H=f.H, W=f.W, dtype=f.dt, ln1=nxt,
                     n_out=w["n2b"], ldn=f.ldc, gap_out=w["gap"], gap_c=gap_c, n16_out=(w["n16"] if self.use_n16 else None),
                     sat=self._sat(hb.out16))
        w["n"], w["n2b"] = w["n2b"], w["n"]      # the kernel reads n with a halo: its output n' is another buffer
        f.t, f.have_n, f.have_n16, f.nblk = tout, True, self.use_n16, ops.ffn_tiles(hb.ffn, f.H, f.W, f.dt)

    def _tail_fused180(self, f: _Fwd, hb: _Hab):
        """embed_dim 180: aggregation + scaled c2 + residuals + the whole FFN in one launch (hat_hab_tail3)."""
        w, t = f.w, f.t
        tout = w["tB"] if t is not w["tB"] else w["tC"]
        nxt, gap_c = hb.next_ln
        ops.hab_tail(hb.ffn3, hb.esc.aggr, t, tout, hb.n2[0], hb.n2[1], n=w["n"], ldn_in=f.ldc, y16=w["y16"], bias_b=hb.bias256,
                     B=f.B, H=f.H, W=f.W, dtype=f.dt, ln1=nxt, n_out=w["n2b"], ldn=f.ldc, gap_out=w["gap"], gap_c=gap_c,
                     n16_out=(w["n16"] if self.use_n16 else None), r2=w["c2"], ldr2=f.ldc, r2scale=w["scale"],
                     r2scale_bstride=hb.cab2.npad)
        w["n"], w["n2b"] = w["n2b"], w["n"]
        f.t, f.have_n, f.have_n16, f.nblk = tout, True, self.use_n16, -(-f.H // 8) * -(-f.W // 16)

    def _tail_aggr_cab(self, f: _Fwd, hb: _Hab):
        """tB = t + aggr(cat(y16, n[pdim:])) + the folded CAB (hat_aggr_cab), then the FFN."""
        w = f.w
        ops.aggr_cab(hb.esc.aggr, w["n"], w["tB"], w["c1"], w["wf"], w["bias_b"], **f.geo, ldx=f.ldc, ldo=self.C, x0=w["y16"],
                     c_split=hb.esc.pdim, ldx0=w["y16"].shape[2], r1=f.t, ldr1=self.C)
        self._ffn(f, hb)

    def _tail_aggr(self, f: _Fwd, hb: _Hab):
        """tB = t + aggr(cat(y16, n[pdim:])) + conv_scale * eca * c2 (hat_linear), then the FFN                  :236"""
        w = f.w
        self._run_lin(hb.esc.aggr, w["n"], w["tB"], **f.geo, ldx=f.ldc, ldo=self.C, out_mode=O_NHWC_F32, x0=w["y16"],
                      c_split=hb.esc.pdim, ldx0=w["y16"].shape[2], r1=f.t, ldr1=self.C, r2=w["c2"], ldr2=f.ldc,
                      r2scale=w["scale"], r2scale_bstride=hb.cab2.npad)
        self._ffn(f, hb)

    def _ffn(self, f: _Fwd, hb: _Hab):
        """The FFN on tB: fused LN2 + fc1 + dw3x3 + gate + fc2 + residual (+ the next block's LayerNorm) -> tC, or the
        unfused LN2, fc1, gate (HATX: SGFN), fc2 in place on tB."""
        w, C, ldc = f.w, self.C, f.ldc
        tB, tC = w["tB"], w["tC"]
        if hb.ffn is not None:
            nxt, gap_c = hb.next_ln
            if gap_c > 16:   # (the fused kernels pool at most 16 channels: a wider ESC gets its LayerNorm + pool from hat_layernorm)
                ops.ffn(hb.ffn, tB, tC, hb.n2[0], hb.n2[1], B=f.B, H=f.H, W=f.W, dtype=f.dt)
                f.t, f.have_n, f.have_n16 = tC, False, False
            else:
                ops.ffn(hb.ffn, tB, tC, hb.n2[0], hb.n2[1], B=f.B, H=f.H, W=f.W, dtype=f.dt, ln1=nxt, n_out=w["n"], ldn=ldc,
                        gap_out=w["gap"], gap_c=gap_c)
                # (hat_ffn / hat_ffn2 emit the LayerNorm rows only: w["n16"] still holds an OLDER block's compact copy —
                # the group conv's or a fused tail's — and must not be handed to the next 13x13 conv)
                f.t, f.have_n, f.have_n16, f.nblk = tC, True, False, ops.ffn_tiles(hb.ffn, f.H, f.W, f.dt)
            return
        f.ln(tB, w["n"], hb.n2)
        hid2 = hb.fc1.nout
        self._run_lin(hb.fc1, w["n"], w["u"], **f.geo, ldx=ldc, ldo=w["u"].shape[2])
        if self.hatx:   # SGFN: [dw(a) * silu(b) | b], hid2 channels in and out            hatx_arch.py:165-177
            ops.sgfn_gate(w["u"], hb.dw_w, hb.dw_b, w["g"], B=f.B, H=f.H, W=f.W, half=hid2 // 2, ldu=w["u"].shape[2],
                          ldo=w["g"].shape[2], dtype=f.dt)
        else:
            ops.dwconv_gate(w["u"], hb.dw_w, hb.dw_b, w["g"], B=f.B, H=f.H, W=f.W, hid=hid2 // 2, ldu=w["u"].shape[2],
                            ldo=w["g"].shape[2], dtype=f.dt)
        self._run_lin(hb.fc2, w["g"], tB, **f.geo, ldx=w["g"].shape[2], ldo=C, out_mode=O_NHWC_F32, r1=tB, ldr1=C)
        f.t, f.have_n, f.have_n16 = tB, False, False

    def _ocab(self, f: _Fwd, G: _Group, as_conv_input):
        """OCAB of residual group G on the residual stream f.t -> the buffer holding the result   hat_arch.py:326-393
        as_conv_input: the only consumer is the group's 3x3 conv, which reads its input as T (bf16) rows anyway: the last
        linear then stores its fp32 result (+ residual) as T rows into w["ao"] and the fp32 stream is not written at all
        (same values as the conv's own staging conversion; 650 B/px less traffic per group)."""
        w, oc, esc, bd, t, C, ldc, geo = f.w, G.ocab, G.ocab.esc, f.band, f.t, self.C, f.ldc, f.geo
        nblk = f.nblk
        if bd is not None:   # key / value windows reach (wse - ws) / 2 rows into the neighbours' bands             :359-360
            # (+ the ESC conv under them with OCAB-ESC).  HATX's focus bias and top-k need nothing more: the saliency head is
            # 1x1 and keys are ranked per window.  A window with owned query rows has its whole key window inside the buffer
            # (ghost 16 >= pad), and the first / last band have the frame edge at their buffer edge, so the padded keys and
            # the lowest-index tie rule are the frame's.
            yield ("halo", [((w["n"] if f.have_n else t), self._ocab_halo(oc))])
        if not f.have_n:
            f.ln(t, w["n"], oc.n1, gap_c=(esc.pdim if esc else 0))
            nblk = ops.layernorm_blocks()
        kv_src = w["n"]
        if esc is not None:  # K/V from ESC(LN(x))                                     :336-344
            if bd is not None:   # the ESC pool over the whole FRAME: this band's rows, then ONE more reduce per group
                gl, gg = f.gstat(esc)
                f.pooled(w["n"], ldc, esc.pdim, gl)
                yield ("reduce", [(gl, gg, esc.pdim)])
                self._esc_w(esc, w, f.B, bd.Hfull, f.W, 1, gap=gg)
                self._esc_conv(esc, w, w["n"], f.B, f.H, f.W)
            else:
                self._esc_lk(esc, w, w["n"], f.B, f.H, f.W, nblk)
            self._run_lin(esc.aggr, w["n"], w["yesc"], **geo, ldx=ldc, ldo=ldc, x0=w["y16"], c_split=esc.pdim, ldx0=w["y16"].shape[2])
            kv_src = w["yesc"]
        if oc.qkvf is not None:
            ops.ocab_qkv(oc.qkvf, w["n"], w["qkv"], **geo, ldx=ldc, ldo=432)
            qbuf, kvbuf, ldq, ldkv = w["qkv"], w["qkv"].view(-1)[144:], 432, 432
        else:
            qbuf, kvbuf, ldq, ldkv = w["q"], w["kv"], ldc, w["kv"].shape[2]
            s0 = torch.cuda.current_stream(self.dev)   # q and kv projections are independent
            s1 = self._side_stream(f)
            s1.wait_stream(s0)
            with torch.cuda.stream(s1):
                self._run_lin(oc.q, w["n"], w["q"], **geo, ldx=ldc, ldo=ldc)
            self._run_lin(oc.kv, kv_src, w["kv"], **geo, ldx=ldc, ldo=w["kv"].shape[2])
            s0.wait_stream(s1)
        self._ocab_attention(f, G, kv_src, qbuf, kvbuf, ldq, ldkv)
        tout = w["tB"] if t is w["tA"] else t  # never write the RHAG input buffer (an FP16 t is hB / hC: proj and MLP take it in place)
        if oc.proj.frag:  # norm2 (:306) rides on the projection's epilogue
            self._run_lin(oc.proj, w["ao"], tout, **geo, ldx=ldc, ldo=C, out_mode=O_NHWC_F32, r1=t, ldr1=C,
                          ln=oc.n2, ln_out=w["n"], ld_ln=ldc, **({"sat": self._sat(True)} if tout.dtype == torch.float16 and self._armed else {}))
        else:
            self._run_lin(oc.proj, w["ao"], tout, **geo, ldx=ldc, ldo=C, out_mode=O_NHWC_F32, r1=t, ldr1=C)
            f.ln(tout, w["n"], oc.n2)
        if oc.mlpf is not None:   # fc1 + GELU + fc2 + residual fused: the hidden tensor never reaches HBM
            dst = w["ao"] if as_conv_input else tout
            ops.ocab_mlp(oc.mlpf, w["n"], tout, dst, B=f.B, H=f.H, W=f.W, ldx=ldc, ldr1=C, ldo=(ldc if as_conv_input else C),
                         out_f32=not as_conv_input, dtype=f.dt)
            return dst
        self._run_lin(oc.mlp0, w["n"], w["g"], **geo, ldx=ldc, ldo=w["g"].shape[2], act=ACT_GELU)
        if as_conv_input:
            self._run_lin(oc.mlp2, w["g"], w["ao"], **geo, ldx=w["g"].shape[2], ldo=ldc, out_mode=O_NHWC_T, r1=tout, ldr1=C)
            return w["ao"]
        self._run_lin(oc.mlp2, w["g"], tout, **geo, ldx=w["g"].shape[2], ldo=C, out_mode=O_NHWC_F32, r1=tout, ldr1=C)
        return tout

    def _ocab_attention(self, f: _Fwd, G: _Group, kv_src, qbuf, kvbuf, ldq, ldkv):
        """Overlapping cross-attention -> w["ao"]; HATX: focus bias on the logits and / or top-k key pruning   hatx_arch.py:421-449"""
        w, oc, C, ldc, ws, wse = f.w, G.ocab, self.C, f.ldc, self.ws, self.wse
        if not (self.focus or self.topk < 1.0):
            ops.ocab_attention(qbuf, kvbuf, oc.bias_rot, w["ao"], B=f.B, H=f.H, W=f.W, C_=C, heads=G.heads, ws=ws, wse=wse,
                               ldq=ldq, ldkv=ldkv, ldo=ldc, dtype=f.dt, q_log2=oc.qlog2)
            return
        nk, pad = wse * wse, (wse - ws + 1) // 2
        if self.focus:
            ops.conv(oc.fh0, kv_src, w["fh"], **f.geo, ldx=ldc, ldo=w["fh"].shape[2], act=ACT_GELU, n_store=_r4(C // 4))
            ops.conv(oc.fh2, w["fh"], w["sal"], **f.geo, ldx=w["fh"].shape[2], ldo=8, n_store=4, out_mode=O_NHWC_F32)
        k_keep = max(1, int(self.topk * nk)) if self.topk < 1.0 else nk
        ops.ocab_keybias(w["sal"] if self.focus else None, kvbuf, w["kb"], B=f.B, H=f.H, W=f.W, C_=C, ws=ws, wse=wse, pad=pad,
                         k_keep=k_keep, ldsal=(-8 if f.dt == ops.HAT_BF16 else 8), ldkv=ldkv, dtype=f.dt)
        ops.ocab_attention_kb(qbuf, kvbuf, oc.bias_rot, w["kb"], w["ao"], B=f.B, H=f.H, W=f.W, C_=C, heads=G.heads, ws=ws,
                              wse=wse, pad=pad, ldq=ldq, ldkv=ldkv, ldo=ldc, dtype=f.dt)

    def _group_end(self, f: _Fwd, G: _Group, tout):
        """RHAG tail: conv3x3 + group residual, written over the group input (or the identity add)           :545-546, :556"""
        w, tA, C = f.w, f.w["tA"], self.C
        if f.band is not None and G.conv is not None:   # the group's 3x3 conv reads one row beyond the band's own
            yield ("halo", [(tout, 1)])
        if G.conv is None:  # resi_connection == 'identity': group(x) + x
            ops.add_f32(tout, tA, tA, B=f.B, n=f.N * C)
            f.t = f.gin = tA
            f.have_n = f.have_n16 = False
            return
        # the epilogue emits the LayerNorm its consumer starts with (the next group's first norm1, or HAT.norm): w["n"] (and
        # w["n16"]) are then already valid when the next step starts
        lnkw = {}
        if G.conv_ln is not None:
            nxt, gap_c = G.conv_ln
            lnkw = dict(ln=nxt, ln_out=w["n"], ld_ln=f.ldc, gap_out=w["gap"], gap_c=gap_c, n16_out=(w["n16"] if self.use_n16 and gap_c else None))
            f.nblk = ops.conv_tiles(G.conv, f.H, f.W, f.dt)
        f.have_n = G.conv_ln is not None
        f.have_n16 = bool(f.have_n and self.use_n16 and G.conv_ln[1])
        gout = w["hA"] if G.out16 else tA   # written over the group input when both have the same type, else into hA
        if G.to_conv:
            ops.conv(G.conv, tout, gout, **f.geo, ldx=f.ldc, ldo=C, x_mode=X_NHWC_T, out_mode=O_NHWC_F32, r1=f.gin, ldr1=C,
                     sat=self._sat(G.out16), **lnkw)
        else:
            ops.conv(G.conv, tout, gout, **f.geo, ldx=C, ldo=C, x_mode=X_NHWC_F32, out_mode=O_NHWC_F32, r1=f.gin, ldr1=C, **lnkw)
        f.t = f.gin = gout

    def _body_end(self, f: _Fwd):
        """final LN; conv_after_body + f0 ; conv_before_upsample + LeakyReLU               :844, :854-855"""
        w, tA, C, ldc = f.w, f.w["tA"], self.C, f.ldc
        if f.gin is not tA and not (f.have_n and self.conv_after_body is not None):
            raise RuntimeError("the FP16 residual stream reached a reader that takes fp32 only")   # (_plan_t16 rules it out)
        if self.conv_after_body is None:   # nn.Identity: LN(t) + f0 in fp32, read as such by the next conv      :748
            if f.band is not None:   # the same one refresh as below: LN + f0 and the four 3x3 convs that end the network read < 4 rows
                yield ("halo", [(tA, 8)])
            f.ln(tA, w["tB"], self.norm, out_f32=True)
            ops.add_f32(w["tB"], w["f0"], w["tB"], B=f.B, n=f.N * C)
            ops.conv(self.conv_before_up, w["tB"], w["fb"], **f.geo, ldx=C, ldo=64, x_mode=X_NHWC_F32, act=ACT_LRELU)
            return
        if f.band is not None:
            # conv_after_body, conv_before_upsample, the Upsample convs and conv_last are five 3x3 convs, the last two at
            # 2x / 4x resolution: their receptive field is < 4 LR rows.  ONE refresh of 8 rows here, then the band computes
            # its ghost rows redundantly (f0 = conv_first(x) is exact there: the band's x carries the ghost rows).
            yield ("halo", [((w["n"] if f.have_n else tA), 8)])
        if not f.have_n:
            f.ln(tA, w["n"], self.norm)
        ops.conv(self.conv_after_body, w["n"], w["c2"], **f.geo, ldx=ldc, ldo=ldc, r1=w["f0"], ldr1=C)
        ops.conv(self.conv_before_up, w["c2"], w["fb"], **f.geo, ldx=ldc, ldo=64, act=ACT_LRELU)

    def _upsample(self, f: _Fwd, y, sink=None):
        """conv + PixelShuffle per stage; conv_last ; / img_range + mean                     :593-605, :856-858
        Where the network ends folded (_folded) the last stage and conv_last are hat_upfold_*, with the same three ways out.
        Without a sink conv_last writes the fp32 planes y.  With one (then y is sink.out) it converts in its epilogue, sink.fused,
        where the row-sweep kernel runs with three output channels; else it writes fp32 planes of its own as always and
        sink.from_planes converts and crops them."""
        src, h, wd, dt = f.w["fb"], f.H, f.W, f.dt
        fold = self._folded(f.W)
        for (pw, rr), dst in list(zip(self.ups, f.w["ups"]))[:len(self.ups) - int(fold)]:
            ops.conv(pw, src, dst, B=f.B, H=h, W=wd, dtype=dt, ldx=64, ldo=64, out_mode=O_PIXSHUF_T, ps_r=rr)
            src, h, wd = dst, h * rr, wd * rr
        r = float(self.cfg.get("img_range", 1.0))
        if fold:   # the last stage and conv_last in one launch on the stage's input: the same epilogue choice as below
            kw = dict(B=f.B, H=h, W=wd, ldx=64, out_scale=1.0 / r, mean=self._mean(), dtype=dt)
            if sink is not None and sink.fusable:
                sink.folded(src, self.upfold, **kw)
                return
            if sink is not None:
                y = torch.empty(f.B, 3, 2 * h, 2 * wd, dtype=torch.float32, device=self.dev)
            ops.upfold_to_planes(src, self.upfold, y, **kw)
            if sink is not None:
                sink.from_planes(y)
            return
        if sink is not None:
            if self.u8_fused and wd % 16 == 0 and sink.fusable:
                wpk, b8, _ = self.conv_last_sweep
                sink.fused(src, wpk, b8, B=f.B, H=h, W=wd, C_=64, ldx=64, out_scale=1.0 / r, mean=self._mean(), dtype=dt)
                return
            y = torch.empty(f.B, 3, h, wd, dtype=torch.float32, device=self.dev)
        if self.conv_last_sweep is not None and wd % 16 == 0:
            wpk, b8, nout = self.conv_last_sweep
            ops.conv3x3_to_planes(src, wpk, b8, y, B=f.B, H=h, W=wd, C_=64, ldx=64, n_out=nout, out_scale=1.0 / r, mean=self._mean(),
                                  dtype=dt)
        else:
            ops.conv(self.conv_last, src, y, B=f.B, H=h, W=wd, dtype=dt, ldx=64, ldo=0, out_mode=O_NCHW_F32,
                     out_scale=1.0 / r, mean=self._mean())
        if sink is not None:
            sink.from_planes(y)
