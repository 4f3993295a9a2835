"""`ESCEngine` — the ESC network (esc_arch.py:301-386) as a launch sequence on the MI355X: packed weights, a workspace per
input shape, no torch op on the hot path.  DESIGN.md §4.14 has the launch list.

The residual stream is fp32 rows (B, H*W, 64); what a 1x1 / 3x3 / 13x13 conv reads is T rows (T = the compute dtype).  Per Block:
    hat_esc_convffn (LN + ConvFFN)  ->  hat_esc_layernorm, to_qkv, hat_window_attention_r, to_out (+ x)
    conv_blocks x [ hat_esc_convffn (+ pool partials), hat_esc_weights, 13x13 conv, aggr (+ x) ]  ->  hat_esc_layernorm, conv_out (+ skip)
One engine runs the whole family: stem, the Block loop, residual, head, with the three parts (esc_parts.py) chosen by the class:
`ESCEngine`, `ESCRealEngine` (§4.15), `ESCRealMEngine` (§4.18), `ESCFPEngine` (§4.16: 48 channels, `WIDTH[48]`'s kernels) and
`ESCLTEEngine` (§4.19: the encoder of the arbitrary-scale model, and the queries on what it left).
"""
from __future__ import annotations

import functools
import types

import torch

from . import ops
from .engine_base import EngineBase
from .esc_parts import (LN_EPS, ConvHead, DySampleHead, Feat0Residual, LTEHead, NearestX4Head, PlainStem, ShuffleAddHead, ShuffleBicubicHead,
                        ShufflePlanesHead, SkipResidual, StepsHead, UnshuffledSkipResidual, UnshuffledStem)
from .frame_boundary import FrameBoundary
from .ops import O_NHWC_F32, O_NHWC_T
from .packing import _ESC

SUPPORTED = dict(dim=64, pdim=16, kernel_size=13, window_size=32, num_heads=4)
FP_SUPPORTED = dict(dim=48, pdim=16, kernel_size=13, window_size=32, num_heads=3)


def _esc_lk(e, sd):
    """-> the packer of a conv block's large-kernel branch.  The geometric re-parameterisation of the one shared filter is done
    here, once, unless convert() has baked it in already."""
    plk = sd["plk_filter"].detach().to(torch.float32).cpu()
    sd = dict(sd, _plk=plk if e.cfg.get("converted", False) else ops.esc_geo_ensemble(plk))
    return lambda core: _ESC(sd, core, "_plk", 16, 13, e.C, e.dtype, e.dev)


def _esc_weights(esc, w, tiles: int, N: int, B: int, dtype):
    """The per-sample weight image of the 13x13 conv, from the pool partials the ConvFFN left."""
    ops.esc_weights(w["gap"], tiles, N, esc.w1, esc.b1, esc.w2, esc.b2, esc.plk, w["weff"], B=B, pdim=16, ksize=13, kpad=esc.kpad, dtype=dtype)


def _escfp_lk(e, sd):   # lk_channel / lk_spatial are used as they are: no geometric ensemble, no convert()
    return lambda core: ops.pack_escfp_lk(sd, core, e.dtype, e.dev)


def _escfp_weights(esc, w, tiles, N, B, dtype):
    ops.escfp_weights(w["gap"], tiles, N, esc, w["weff"], B=B, dtype=dtype)


# what the width of the body swaps: the two kernels that are instantiated per channel count, their packer, and the large-kernel branch
WIDTH = {64: types.SimpleNamespace(convffn=ops.esc_convffn, layernorm=ops.esc_layernorm, pack_ffn=ops.pack_esc_convffn, lk=_esc_lk,
                                   weights=_esc_weights),
         48: types.SimpleNamespace(convffn=ops.escfp_convffn, layernorm=ops.escfp_layernorm, pack_ffn=ops.pack_escfp_convffn, lk=_escfp_lk,
                                   weights=_escfp_weights)}


def _check_esc(cfg):
    for k, v in SUPPORTED.items():
        if int(cfg[k]) != v:
            raise ValueError(f"ESC with {k}={cfg[k]} is not supported: the device path is built for "
                             + ", ".join(f"{a}={b}" for a, b in SUPPORTED.items()) + " (ESC, ESC-light, ESCReal's body)")
    if int(cfg["dim"] * cfg["exp_ratio"]) not in ops.ESC_HID_PAD:
        raise ValueError(f"ESC with exp_ratio={cfg['exp_ratio']} is not supported: hat_esc_convffn is built for exp_ratio 1.25 and 2")


class ESCEngine(FrameBoundary, EngineBase):
    """The frame boundary (frame_boundary.FrameBoundary: bytes, ground truth, YCbCr, the self-ensemble) is mixed in with two hooks
    of its own: a frame is not padded (the window attention reflects its own edges, the unshuffled stem pads itself), and the
    factor between a frame and its result is the one the stem and the head really apply.  DESIGN.md §4.21."""
    WS_MAX = 4   # entries of the workspace LRU

    def __init__(self, cfg: dict, sd: dict, device, compute_dtype: str = "bf16"):
        _check_esc(cfg)
        self._build(cfg, sd, device, compute_dtype, PlainStem, Feat0Residual, ShuffleAddHead)

    def _build(self, cfg, sd, device, compute_dtype, stem, residual, head, batches: bool = False):
        """The one constructor: the body's packing, then the parts, each made as part(self, sd)."""
        if compute_dtype not in ops.DTYPE_CODE:
            raise ValueError(f"compute_dtype {compute_dtype!r}: expected 'bf16' or 'fp32'")
        super().__init__(device, compute_dtype, self.WS_MAX)   # (a host device is taken: the engine then packs and never runs)
        self.cfg, dt, self.batches = dict(cfg, in_chans=3), self.dtype, batches
        self.u8_fused_calls = self.u8_planes_calls = 0   # 8-bit forwards that ended in a fused sink / in hat_planes_to_u8
        self.yuv_fused_calls = self.yuv_planes_calls = 0   # YCbCr forwards that ended in a fused sink / in hat_planes_to_yuv
        self.C, self.scale, self.heads, self.ws = int(cfg["dim"]), int(cfg["upscaling_factor"]), int(cfg["num_heads"]), int(cfg["window_size"])
        dev, C = self.dev, self.C
        wd = self.width = WIDTH[C]
        vec = lambda k: sd[k].detach().to(dtype=torch.float32, device=dev).contiguous()
        pack_lk = wd.lk(self, sd)
        self.blocks = []
        for i in range(int(cfg["n_blocks"])):
            p, b = f"blocks.{i}", types.SimpleNamespace()
            b.ln_proj = (vec(p + ".ln_proj.weight"), vec(p + ".ln_proj.bias"))
            b.proj = wd.pack_ffn(sd, p + ".proj", dt, dev)
            b.ln_attn = (vec(p + ".ln_attn.weight"), vec(p + ".ln_attn.bias"))
            # head_dim^-0.5 = 1/4 folded into the q rows of to_qkv: a power of two, so exact
            qs = torch.cat([torch.full((C,), (C // self.heads) ** -0.5), torch.ones(2 * C)])
            wq = sd[p + ".attn.to_qkv.weight"].detach().to(torch.float32).cpu().reshape(3 * C, C) * qs[:, None]
            bq = sd[p + ".attn.to_qkv.bias"].detach().to(torch.float32).cpu() * qs
            b.to_qkv = ops.pack_pointwise(wq, bq, dt, dev)
            b.to_out = ops.pack_pointwise(sd[p + ".attn.to_out.weight"].detach().reshape(C, C), sd[p + ".attn.to_out.bias"], dt, dev)
            b.rpb = vec(p + ".attn.relative_position_bias")
            b.convs = []
            for j in range(int(cfg["conv_blocks"])):
                ln = (vec(f"{p}.lns.{j}.weight"), vec(f"{p}.lns.{j}.bias")) if cfg.get("use_ln", False) else None
                esc = pack_lk(f"{p}.pconvs.{j}")
                esc.aggr = ops.pack_pointwise(sd[f"{p}.pconvs.{j}.aggr.weight"].detach().reshape(C, C), sd[f"{p}.pconvs.{j}.aggr.bias"], dt, dev)
                esc.conv13 = ops.esc_conv13_supported(16, 13, dt)
                b.convs.append((ln, wd.pack_ffn(sd, f"{p}.convffns.{j}", dt, dev), esc))
            b.ln_out = (vec(p + ".ln_out.weight"), vec(p + ".ln_out.bias"))
            b.conv_out = ops.pack_conv_weight(sd[p + ".conv_out.weight"], sd[p + ".conv_out.bias"], dt, dev)
            self.blocks.append(b)
        self.last = ops.pack_conv_weight(sd["last.weight"], sd["last.bias"], dt, dev)
        self._kpad = self.blocks[0].convs[0][2].kpad if self.blocks and self.blocks[0].convs else 0
        self.stem, self.residual, self.head = stem(self, sd), residual(self, sd), head(self, sd)

    def _check_batch(self, B: int):
        if B != 1 and not self.batches:
            raise RuntimeError("ESC's eval path takes one frame at a time (esc_arch.py:121: the dynamic kernel of a batch cannot be "
                               f"reshaped to (pdim,1,3,3)), got a batch of {B}")

    def _body_size(self, h: int, w: int):
        return self.stem.body_size(h, w)

    def _check_frame(self, H: int, W: int):
        self.residual.check_frame(H, W)

    def _alloc_workspace(self, B: int, h: int, w: int, tag=None):
        """Keyed by the frame's shape (EngineBase._workspace); the buffers have the body's size."""
        H, W = self._body_size(h, w)
        dev, N, C = self.dev, H * W, self.C
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        t = lambda *shape: torch.zeros(*shape, dtype=self.tdt, device=dev)
        w = {"feat0": f(B, N, C), "s": [f(B, N, C) for _ in range(3)], "n": t(B, N, C), "qkv": t(B, N, 3 * C), "att": t(B, N, C),
             "z": t(B, N, C), "y16": t(B, N, 16), "gap": f(B, ops.esc_convffn_tiles(H, W), 16), "weff": t(B, 16, max(self._kpad, 1))}
        for part in (self.stem, self.residual, self.head):
            w.update(part.buffers(B, H, W, f, t))
        return w

    def _lin(self, pw, x, out, *, geo, ldx, ldo, out_mode=O_NHWC_T, **kw):
        if pw.frag:
            ops.linear(pw, x, out, **geo, dtype=self.dtype, ldx=ldx, ldo=ldo, out_mode=out_mode, **kw)
        else:
            ops.conv(pw, x, out, **geo, dtype=self.dtype, ldx=ldx, ldo=ldo, out_mode=out_mode, **kw)

    def _pad_multiple(self) -> int:
        return 1   # any frame size is taken as it is; _check_input refuses what the reflections cannot serve

    def _out_factor(self) -> int:
        """What the network applies to a frame: behind an unshuffled stem the x4 head runs on a smaller body and the result is the
        (s h, s w) corner of its buffer; else the head's own factor where it has one (ESCReal's default head: 4)."""
        return self.scale if self.stem.f else (self.head.out_scale or self.scale)

    def _check_input(self, x):
        """The shapes every forward refuses (_forward calls it; an ensemble calls it before it allocates or launches)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"ESC expects (B,3,h,w) input, got {tuple(x.shape)}")
        self._check_batch(x.shape[0])
        H, W = self._body_size(x.shape[2], x.shape[3])
        ws = self.ws
        if (-H) % ws > H - 1 or (-W) % ws > W - 1:
            raise RuntimeError(f"a {H}x{W} frame cannot be reflect-padded to a multiple of window_size {ws}: the padding must be smaller than the frame")
        self._check_frame(H, W)

    def _forward(self, x: torch.Tensor, one_stream=None, sink=None, taps: dict = None) -> torch.Tensor:
        """x (B, 3, h, w) fp32 (B = 1 unless the network takes batches) -> (B, 3, s h, s w) fp32 (the workspace's output buffer: copy it before the next forward of the shape).
        one_stream: accepted and ignored (there is no side stream).  sink (a frame_boundary._Sink): the head fills and returns
        sink.out, bytes, instead of fp32 planes.
        taps: a dict that receives clones of the stream after the first ConvFFN, the attention and the first conv block."""
        self._check_input(x)
        B, _, h0, w0 = x.shape
        H, W = self._body_size(h0, w0)
        ws = self.ws
        x = x.to(torch.float32).contiguous()
        w, C, dt, N = self._workspace(B, h0, w0), self.C, self.dtype, H * W
        geo = dict(B=B, H=H, W=W)
        tiles = w["gap"].shape[1]
        wd = self.width
        self.stem.run(x, w, geo)
        cur = w["feat0"]
        for bi, b in enumerate(self.blocks):
            xa, xb = [s for s in w["s"] if s is not cur][:2]
            wd.convffn(b.proj, cur, xa, **geo, dtype=dt, ln=b.ln_proj, eps=LN_EPS, ldx=C, ldo=C)
            if taps is not None and bi == 0:
                taps["ffn0"] = xa.clone()
            wd.layernorm(xa, w["n"], *b.ln_attn, npix=B * N, dtype=dt, eps=LN_EPS, ldx=C, ldy=C)
            self._lin(b.to_qkv, w["n"], w["qkv"], geo=geo, ldx=C, ldo=3 * C)
            ops.window_attention_r(w["qkv"], w["qkv"].view(-1)[C:], b.rpb, w["att"], B=B, h=H, w=W, C_=C, heads=self.heads, ws=ws,
                                   ldq=3 * C, ldkv=3 * C, ldo=C, dtype=dt)
            self._lin(b.to_out, w["att"], xb, geo=geo, ldx=C, ldo=C, out_mode=O_NHWC_F32, r1=xa, ldr1=C)
            xa, xb = xb, xa
            if taps is not None and bi == 0:
                taps["attn0"] = xa.clone()
            for ci, (ln, ffn, esc) in enumerate(b.convs):
                wd.convffn(ffn, xa, w["z"], **geo, dtype=dt, ln=ln, eps=LN_EPS, partials=w["gap"], ldx=C, ldo=C)
                wd.weights(esc, w, tiles, N, B, dt)
                if esc.conv13:
                    ops.esc_conv13(w["z"], w["weff"], w["y16"], **geo, ldx=C, kpad=esc.kpad, dtype=dt)
                else:
                    pw = ops.PackedConv(w["weff"], esc.zero_bias, 13, 16, esc.kpad, 1, 1, 16, w_bstride=16 * esc.kpad)
                    ops.conv(pw, w["z"], w["y16"], **geo, dtype=dt, ldx=C, ldo=16, n_store=16)
                self._lin(esc.aggr, w["z"], xb, geo=geo, ldx=C, ldo=C, out_mode=O_NHWC_F32, x0=w["y16"], c_split=16, ldx0=16, r1=xa, ldr1=C)
                xa, xb = xb, xa
                if taps is not None and bi == 0 and ci == 0:
                    taps["conv0"] = xa.clone()
            wd.layernorm(xa, w["n"], *b.ln_out, npix=B * N, dtype=dt, eps=LN_EPS, ldx=C, ldy=C)
            ops.conv(b.conv_out, w["n"], xb, **geo, dtype=dt, ldx=C, ldo=C, out_mode=O_NHWC_F32, r1=cur, ldr1=C)
            cur = xb
        res = self.residual.run(x, w, cur, geo)
        return self.head.run(x, w, cur, res, geo, sink=sink)


class ESCRealEngine(ESCEngine):
    """ESCReal (esc_real_arch.py:402-475): ESC's body with use_ln, the skip residual (hat_escreal_skip), and the default x4 head or
    DySample (esc_parts.NearestX4Head / DySampleHead).  DESIGN.md §4.15."""

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        _check_esc(cfg)
        head, s = NearestX4Head, int(cfg["upscaling_factor"])
        if cfg.get("use_dysample", False):
            if s not in (2, 3, 4):
                raise ValueError(f"ESCReal with use_dysample and upscaling_factor={s} is not supported: hat_dysample is built for 2, 3 and 4")
            head = functools.partial(DySampleHead, out_scale=s, at="to_img", pre=False)
        self._build(cfg, sd, device, compute_dtype, PlainStem, functools.partial(SkipResidual, what="frame"), head)


class ESCRealMEngine(ESCEngine):
    """ESCRealM (esc_real_arch.py:478-661): ESCReal's body and residual, with
        unshuffle mode   the unshuffled stem and its skip residual (esc_parts.UnshuffledStem / UnshuffledSkipResidual); the body runs
                         at ceil(h/f) x ceil(w/f), the head is x4 and the output is the (s h, s w) corner of its buffer
        plain mode       ESCReal's stem and residual
    and UniUpsample's five heads at the internal scale S (4 in unshuffle mode, else upscaling_factor): "conv" (ConvHead, also any
    upsampler at S = 1), "pixelshuffledirect" (ShufflePlanesHead), "pixelshuffle" and "nearest+conv" (StepsHead), "dysample"
    (DySampleHead, behind to_img.0 when mid_dim != dim).  DESIGN.md §4.18."""

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        _check_esc(cfg)
        s, up, mid = int(cfg["upscaling_factor"]), cfg["upsampler"], int(cfg["mid_dim"])
        S = int(cfg["head_scale"])
        if up not in ops.UNI_UPSAMPLERS:
            raise ValueError(f"ESCRealM with upsampler={up!r} is not supported: expected one of {ops.UNI_UPSAMPLERS}")
        if s not in (1, 2, 3, 4) or S not in (1, 2, 3, 4):
            raise ValueError(f"ESCRealM with upscaling_factor={s} is not supported: the heads are built for 1, 2, 3 and 4")
        if cfg["unshuffle"] and up == "conv":
            raise ValueError("ESCRealM with upsampler='conv' behind the unshuffled stem is not supported: its output would be smaller than the frame")
        if up == "pixelshuffle" and S > 1 and (mid < 16 or mid % 16):
            raise ValueError(f"ESCRealM with upsampler='pixelshuffle' and mid_dim={mid} is not supported: mid_dim must be a multiple of 16")
        if up == "dysample" and S > 1 and mid not in (48, 64):
            raise ValueError(f"ESCRealM with upsampler='dysample' and mid_dim={mid} is not supported: built for mid_dim 48 and 64")
        part, f = functools.partial, int(cfg["unshuffle"])
        self.f = f
        if S == 1 or up == "conv":
            head = ConvHead
        elif up == "pixelshuffledirect":
            head = part(ShufflePlanesHead, out_scale=S)
        elif up == "dysample":
            pre = mid != int(cfg["dim"]) and mid
            head = part(DySampleHead, out_scale=S, at="to_img.2" if pre else "to_img.0", pre=pre)
        else:
            head = part(StepsHead, out_scale=S, nearest=up == "nearest+conv", mid=mid)
        self._build(cfg, sd, device, compute_dtype, part(UnshuffledStem, f=f) if f else PlainStem,
                    part(UnshuffledSkipResidual, what="map", behind=f" behind the /{f} unshuffle") if f else part(SkipResidual, what="map"), head)

    def _forward(self, x, one_stream=None, sink=None, taps=None):
        y = super()._forward(x, sink=sink, taps=taps)
        if self.f and sink is None:   # the reference's crop to (s h, s w): a corner of the x4 buffer (a sink's size is that crop)
            s = self.scale
            return y[:, :, :s * x.shape[2], :s * x.shape[3]]
        return y


class ESCFPEngine(ESCEngine):
    """ESCFP (esc_fp_arch.py:277-355): ESC's Block loop at 48 channels and 3 heads, with a LayerNorm in front of every conv block,
    hat_escfp_weights in place of hat_esc_weights (the decomposed large-kernel branch folded to the dense rank-1 filter the 13x13
    conv kernels read), then
        hat_escfp_layernorm (ln_last)  ->  last (+ feat0)  ->  to_img  ->  hat_escfp_shuffle_bicubic     (esc_parts.ShuffleBicubicHead)
    Batches are taken: workspace, pool partials and weight images are per sample.  DESIGN.md §4.16."""

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        for k, v in FP_SUPPORTED.items():
            if int(cfg[k]) != v:
                raise ValueError(f"ESCFP with {k}={cfg[k]} is not supported: the device path is built for "
                                 + ", ".join(f"{a}={b}" for a, b in FP_SUPPORTED.items()) + " (ESC_FP_X2 / X3 / X4)")
        if int(cfg["dim"] * cfg["exp_ratio"]) not in ops.ESCFP_HID_PAD:
            raise ValueError(f"ESCFP with exp_ratio={cfg['exp_ratio']} is not supported: hat_escfp_convffn is built for a hidden width of "
                             + ", ".join(map(str, ops.ESCFP_HID_PAD)) + " (exp_ratio 1.25, 1.5, 2)")
        if int(cfg["upscaling_factor"]) not in (2, 3, 4):
            raise ValueError(f"ESCFP with upscaling_factor={cfg['upscaling_factor']} is not supported: hat_escfp_shuffle_bicubic is built for 2, 3 and 4")
        self._build(cfg, sd, device, compute_dtype, PlainStem, Feat0Residual, ShuffleBicubicHead, batches=True)


class ESCLTEEngine(ESCEngine):
    """ESC-LTE (esc_arb/models/lte.py, esc.py): ESC's Block loop as the encoder (no to_img; the geometric filter ensemble on every
    forward), then
        last (+ feat0)  ->  hat_conv 64 -> 512 (coef | freq, fp32 rows)         gen_feat, kept in the workspace of the shape
        hat_lte_query                                                           query / query_grid, any number of times
    The state dict is the reference LTE's: the encoder's keys under `encoder.`, the head's beside them.  DESIGN.md §4.19."""

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        _check_esc(cfg)
        hd, hl = int(cfg.get("hidden_dim", 256)), tuple(int(v) for v in cfg.get("hidden_list", (256, 256, 256)))
        if hd != ops.LTE_HIDDEN or hl != (ops.LTE_HIDDEN,) * 3:
            raise ValueError(f"ESC-LTE with hidden_dim={hd}, hidden_list={hl} is not supported: hat_lte_query is built for hidden_dim "
                             f"{ops.LTE_HIDDEN} and hidden_list {(ops.LTE_HIDDEN,) * 3}")
        sd = dict(sd)
        for k in [k for k in sd if k.startswith("encoder.")]:   # the plain-named keys the shared packing reads
            sd[k[len("encoder."):]] = sd[k]
        self._feat_ws = None
        self._build(dict(cfg, upscaling_factor=1), sd, device, compute_dtype, PlainStem, Feat0Residual, LTEHead)
        self.lte = self.head.lte

    def _no_frame_boundary(self, *a, **k):
        raise RuntimeError("ESC-LTE's forward returns feature rows, not an image: the fixed-scale frame boundary does not apply; its frame "
                           "paths are gen_feat_frame with query_grid_u8 / query_grid_yuv (ESCLTE.upscale_u8 / upscale_yuv)")

    forward_ensemble = forward_to_u8 = forward_u8 = forward_gt_u8 = forward_yuv420 = forward_yuv = _no_frame_boundary

    def _query(self, out, *dst, fn=ops.lte_query, **kw):
        """One launch of hat_lte_query, or of the sink `fn` of its family, on what the last gen_feat left."""
        if self._feat_ws is None:
            raise RuntimeError("ESC-LTE: query before gen_feat: there are no features to query")
        w, H, W = self._feat_ws
        hd = ops.LTE_HIDDEN
        with self._lock, torch.cuda.device(self.dev):
            fn(self.lte, w["cf"], w["cf"].view(-1)[hd:], w["x"], out, *dst, H=H, W=W, ldc=2 * hd, ldf=2 * hd, dtype=self.dtype, **kw)
        return out

    def query(self, coord: torch.Tensor, cell: torch.Tensor) -> torch.Tensor:
        """coord, cell (Q,2) fp32 on the engine's device -> (Q,3) fp32 (a fresh tensor) against the last gen_feat."""
        for name, t in (("coord", coord), ("cell", cell)):
            if t.device != self.dev or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2:
                raise RuntimeError(f"ESC-LTE: {name} must be a (Q,2) fp32 tensor on {self.dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        if coord.shape != cell.shape:
            raise RuntimeError(f"ESC-LTE: coord {tuple(coord.shape)} and cell {tuple(cell.shape)} differ in shape")
        out = torch.empty(coord.shape[0], 3, dtype=torch.float32, device=self.dev)
        if coord.shape[0] == 0:
            return out
        return self._query(out, coord=coord.contiguous(), cell=cell.contiguous())

    def query_grid(self, h: int, w: int, cell_yx, out_affine=(1.0, 0.0)) -> torch.Tensor:
        """The make_coord grid of an (h, w) image, every query with the cell cell_yx -> (3,h,w) fp32 planes * a + b (a fresh tensor)."""
        out = torch.empty(3, h, w, dtype=torch.float32, device=self.dev)
        return self._query(out, grid=(h, w), cell_yx=cell_yx, out_affine=out_affine)

    # ---- frames: 8-bit and YCbCr in, any size out.  The sinks are hat_lte_query's own, so nothing of FrameBoundary
    # (reflect-padding, conv_last's epilogues, the ensemble) applies: ESC's window attention reflects its own edges.
    def _ws_f32(self, H: int, W: int, key: str, shape, dtype=torch.float32) -> torch.Tensor:
        """An fp32 buffer (or one of `dtype`) in the workspace of the (1, H, W) frame shape, allocated with its first use
        (FrameBoundary._ws_buffer's rule)."""
        ws = self._workspace(1, H, W)
        t = ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = ws[key] = torch.zeros(shape, dtype=dtype, device=self.dev)
            ws["bytes"] += t.numel() * t.element_size()
        return t

    def gen_feat_frame(self, H: int, W: int, fill) -> None:
        """gen_feat of a frame that arrives as bytes: fill(x) writes its [0, 1] planes into x (1,3,H,W), the staging buffer of the
        shape's workspace; the normalisation (x - 0.5) / 0.5 runs in place; then the encoder."""
        with self._lock, torch.cuda.device(self.dev):
            x = self._ws_f32(H, W, "x_frame", (1, 3, H, W))
            fill(x)
            x.sub_(0.5).div_(0.5)
            self._forward(x)

    def planes_buffer(self, H: int, W: int, h: int, w: int) -> torch.Tensor:
        """The (1,3,h,w) fp32 image a co-sited YCbCr output is converted from, in the workspace of the (H, W) frame."""
        with self._lock, torch.cuda.device(self.dev):
            return self._ws_f32(H, W, "y_frame", (1, 3, h, w))

    def query_grid_planes(self, out: torch.Tensor, cell_yx, out_affine=(1.0, 0.0)) -> torch.Tensor:
        """query_grid into the caller's (3,h,w) or (1,3,h,w) contiguous fp32 tensor."""
        return self._query(out, grid=tuple(out.shape[-2:]), cell_yx=cell_yx, out_affine=out_affine)

    # ---- the benchmark loop (esc_arb/test.py eval_psnr): the LR frame and the score are made on the device
    def pil_lr_frame(self, gt: torch.Tensor, h_lr: int, w_lr: int) -> torch.Tensor:
        """Pillow's 8-bit bicubic resize of the (h,w,3) uint8 ground truth (rows may be pitched) to (h_lr, w_lr), into the workspace
        of the (h_lr, w_lr) frame (hat_pil_resize_u8)."""
        with self._lock, torch.cuda.device(self.dev):
            return ops.pil_resize_u8(gt, (h_lr, w_lr), dst=self._ws_f32(h_lr, w_lr, "lr_frame", (h_lr, w_lr, 3), torch.uint8))

    def score_grid(self, gt: torch.Tensor, cell_yx, mode, shave: int):
        """The grid of gt's (h, w) against the last gen_feat, image * 0.5 + 0.5, into the workspace; then hat_arb_psnr against gt
        (h,w,3) uint8 -> (sum of squares, number of terms) as Python numbers: sixteen bytes leave the device."""
        if self._feat_ws is None:
            raise RuntimeError("ESC-LTE: score_grid before gen_feat: there are no features to query")
        _, H, W = self._feat_ws
        h, w = int(gt.shape[0]), int(gt.shape[1])
        planes = self.query_grid_planes(self.planes_buffer(H, W, h, w), cell_yx, out_affine=(0.5, 0.5))
        with self._lock, torch.cuda.device(self.dev):
            s = ops.arb_psnr(planes, gt, mode=mode, shave=shave).cpu()
        return float(s[0]), int(s[1])

    def query_grid_u8(self, out: torch.Tensor, cell_yx, bgr: bool = False, out_affine=(0.5, 0.5)) -> torch.Tensor:
        """The grid of out's (h, w) -> out (1,h,w,3) uint8 (rows may be pitched): tensor2img's bytes of the image * a + b."""
        return self._query(out, fn=ops.lte_query_u8, grid=tuple(out.shape[-3:-1]), cell_yx=cell_yx, out_affine=out_affine, bgr=bgr)

    def query_grid_yuv(self, out_views, cell_yx, from_rgb, sub, depth: int = 8, msb=False, out_affine=(0.5, 0.5)) -> None:
        """The grid of the Y view's (h, w) -> the views (y, cb, cr) of a centre-sited frame (ops.yuv_views) of the image * a + b."""
        y, cb, cr = out_views
        self._query(y, cb, cr, from_rgb, fn=ops.lte_query_yuv, grid=tuple(y.shape[-2:]), cell_yx=cell_yx, out_affine=out_affine, sub=sub,
                    depth=depth, msb=msb)
