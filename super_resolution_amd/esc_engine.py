"""`ESCEngine` — the ESC network (esc_arch.py:301-386) as a launch sequence on the MI355X: packed weights, a workspace per
input shape, no torch op on the hot path.  DESIGN.md §4.14 has the launch list.

The residual stream is fp32 rows (B, H*W, 64); what a 1x1 / 3x3 / 13x13 conv reads is T rows (T = the compute dtype).  Per Block:
    hat_esc_convffn (LN + ConvFFN)  ->  hat_esc_layernorm, to_qkv, hat_window_attention_r, to_out (+ x)
    conv_blocks x [ hat_esc_convffn (+ pool partials), hat_esc_weights, 13x13 conv, aggr (+ x) ]  ->  hat_esc_layernorm, conv_out (+ skip)
`ESCRealEngine` (§4.15), `ESCRealMEngine` (§4.18), `ESCLTEEngine` (§4.19: the encoder of the arbitrary-scale model; its head is one
kernel, `hat_lte_query`) and `ESCFPEngine` (§4.16: 48 channels, its own ConvFFN / LayerNorm instantiations and weights launch) reuse
the loop through the hooks of `ESCEngine`.
"""
from __future__ import annotations

import torch

from . import ops
from .engine_base import EngineBase
from .ops import ACT_LRELU, ACT_LRELU02, O_NCHW_F32, O_NHWC_F32, O_NHWC_T, O_PIXSHUF_T, X_NCHW_F32_MEAN, X_NHWC_F32
from .packing import _ESC

LN_EPS = 1e-6   # esc_arch.py:69
SUPPORTED = dict(dim=64, pdim=16, kernel_size=13, window_size=32, num_heads=4)


def _r4(n: int) -> int:
    return (n + 3) // 4 * 4


class _Block:
    pass


class ESCEngine(EngineBase):
    WS_MAX = 4   # entries of the workspace LRU
    # what a width of the family swaps: the two kernels that are instantiated per channel count, and their packer
    _convffn, _layernorm, _pack_ffn = staticmethod(ops.esc_convffn), staticmethod(ops.esc_layernorm), staticmethod(ops.pack_esc_convffn)

    def _check_cfg(self, cfg):
        for k, v in SUPPORTED.items():
            if int(cfg[k]) != v:
                raise ValueError(f"ESC with {k}={cfg[k]} is not supported: the device path is built for "
                                 + ", ".join(f"{a}={b}" for a, b in SUPPORTED.items()) + " (ESC, ESC-light, ESCReal's body)")
        if int(cfg["dim"] * cfg["exp_ratio"]) not in ops.ESC_HID_PAD:
            raise ValueError(f"ESC with exp_ratio={cfg['exp_ratio']} is not supported: hat_esc_convffn is built for exp_ratio 1.25 and 2")

    def __init__(self, cfg: dict, sd: dict, device, compute_dtype: str = "bf16"):
        self._check_cfg(cfg)
        if compute_dtype not in ops.DTYPE_CODE:
            raise ValueError(f"compute_dtype {compute_dtype!r}: expected 'bf16' or 'fp32'")
        super().__init__(device, compute_dtype, self.WS_MAX)   # (a host device is taken: the engine then packs and never runs)
        self.cfg, dt = dict(cfg), self.dtype
        self.C, self.scale, self.heads, self.ws = int(cfg["dim"]), int(cfg["upscaling_factor"]), int(cfg["num_heads"]), int(cfg["window_size"])
        dev, C = self.dev, self.C
        vec = lambda k: sd[k].detach().to(dtype=torch.float32, device=dev).contiguous()
        sd = self._shared_filter(sd)
        self.proj = ops.pack_conv_weight(sd["proj.weight"], sd["proj.bias"], dt, dev)
        self.blocks = []
        for i in range(int(cfg["n_blocks"])):
            p, b = f"blocks.{i}", _Block()
            b.ln_proj = (vec(p + ".ln_proj.weight"), vec(p + ".ln_proj.bias"))
            b.proj = self._pack_ffn(sd, p + ".proj", dt, dev)
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
                esc = self._pack_lk(sd, f"{p}.pconvs.{j}")
                esc.aggr = ops.pack_pointwise(sd[f"{p}.pconvs.{j}.aggr.weight"].detach().reshape(C, C), sd[f"{p}.pconvs.{j}.aggr.bias"], dt, dev)
                esc.conv13 = ops.esc_conv13_supported(16, 13, dt)
                b.convs.append((ln, self._pack_ffn(sd, f"{p}.convffns.{j}", dt, dev), esc))
            b.ln_out = (vec(p + ".ln_out.weight"), vec(p + ".ln_out.bias"))
            b.conv_out = ops.pack_conv_weight(sd[p + ".conv_out.weight"], sd[p + ".conv_out.bias"], dt, dev)
            self.blocks.append(b)
        self.last = ops.pack_conv_weight(sd["last.weight"], sd["last.bias"], dt, dev)
        self._pack_head(sd)
        self._kpad = self.blocks[0].convs[0][2].kpad if self.blocks and self.blocks[0].convs else 0

    def _shared_filter(self, sd):
        """The geometric re-parameterisation of the one large-kernel filter, once, unless convert() has baked it in already."""
        plk = sd["plk_filter"].detach().to(torch.float32).cpu()
        return dict(sd, _plk=plk if self.cfg.get("converted", False) else ops.esc_geo_ensemble(plk))

    def _pack_lk(self, sd, core: str):
        return _ESC(sd, core, "_plk", 16, 13, self.C, self.dtype, self.dev)

    def _lk_weights(self, esc, w, tiles: int, N: int, B: int):
        """The per-sample weight image of the 13x13 conv, from the pool partials the ConvFFN left."""
        ops.esc_weights(w["gap"], tiles, N, esc.w1, esc.b1, esc.w2, esc.b2, esc.plk, w["weff"], B=B, pdim=16, ksize=13, kpad=esc.kpad,
                        dtype=self.dtype)

    def _check_batch(self, B: int):
        if B != 1:
            raise RuntimeError("ESC's eval path takes one frame at a time (esc_arch.py:121: the dynamic kernel of a batch cannot be "
                               f"reshaped to (pdim,1,3,3)), got a batch of {B}")

    def _pack_head(self, sd):
        self.to_img = ops.pack_conv_weight(sd["to_img.weight"], sd["to_img.bias"], self.dtype, self.dev)

    def _head_buffers(self, B: int, H: int, W: int, f, t) -> dict:
        """What the end of the network needs beside the body's buffers; f / t allocate fp32 / T tensors."""
        s = self.scale
        return {"rows": f(B, H * W, _r4(3 * s * s)), "y": f(B, 3, H * s, W * s)}

    # ------------------------------------------------------------------------------------------
    def _body_size(self, h: int, w: int):
        """The size the body runs at for an (h, w) frame: the frame's own, unless a stem shrinks it."""
        return h, w

    def _stem(self, x, w, geo):
        """feat0 = proj(x)"""
        ops.conv(self.proj, x, w["feat0"], **geo, dtype=self.dtype, ldx=0, ldo=self.C, x_mode=X_NCHW_F32_MEAN, out_mode=O_NHWC_F32)

    def _alloc_workspace(self, B: int, h: int, w: int, tag=None):
        """Keyed by the frame's shape (EngineBase._workspace); the buffers have the body's size."""
        H, W = self._body_size(h, w)
        dev, N, C = self.dev, H * W, self.C
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        t = lambda *shape: torch.zeros(*shape, dtype=self.tdt, device=dev)
        w = {"feat0": f(B, N, C), "s": [f(B, N, C) for _ in range(3)], "n": t(B, N, C), "qkv": t(B, N, 3 * C), "att": t(B, N, C),
             "z": t(B, N, C), "y16": t(B, N, 16), "gap": f(B, ops.esc_convffn_tiles(H, W), 16), "weff": t(B, 16, max(self._kpad, 1))}
        w.update(self._head_buffers(B, H, W, f, t))
        return w

    def _lin(self, pw, x, out, *, geo, ldx, ldo, out_mode=O_NHWC_T, **kw):
        if pw.frag:
            ops.linear(pw, x, out, **geo, dtype=self.dtype, ldx=ldx, ldo=ldo, out_mode=out_mode, **kw)
        else:
            ops.conv(pw, x, out, **geo, dtype=self.dtype, ldx=ldx, ldo=ldo, out_mode=out_mode, **kw)

    def _forward(self, x: torch.Tensor, taps: dict = None) -> torch.Tensor:
        """x (B, 3, h, w) fp32 (B = 1 unless the network takes batches) -> (B, 3, s h, s w) fp32 (the workspace's output buffer: copy it before the next forward of the shape).
        taps: a dict that receives clones of the stream after the first ConvFFN, the attention and the first conv block."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"ESC expects (B,3,h,w) input, got {tuple(x.shape)}")
        B, _, h0, w0 = x.shape
        self._check_batch(B)
        H, W = self._body_size(h0, w0)
        ws = self.ws
        if (-H) % ws > H - 1 or (-W) % ws > W - 1:
            raise RuntimeError(f"a {H}x{W} frame cannot be reflect-padded to a multiple of window_size {ws}: the padding must be smaller than the frame")
        self._check_frame(H, W)
        x = x.to(torch.float32).contiguous()
        w, C, dt, N = self._workspace(B, h0, w0), self.C, self.dtype, H * W
        geo = dict(B=B, H=H, W=W)
        tiles = w["gap"].shape[1]
        self._stem(x, w, geo)
        cur = w["feat0"]
        for bi, b in enumerate(self.blocks):
            xa, xb = [s for s in w["s"] if s is not cur][:2]
            self._convffn(b.proj, cur, xa, **geo, dtype=dt, ln=b.ln_proj, eps=LN_EPS, ldx=C, ldo=C)
            if taps is not None and bi == 0:
                taps["ffn0"] = xa.clone()
            self._layernorm(xa, w["n"], *b.ln_attn, npix=B * N, dtype=dt, eps=LN_EPS, ldx=C, ldy=C)
            self._lin(b.to_qkv, w["n"], w["qkv"], geo=geo, ldx=C, ldo=3 * C)
            ops.window_attention_r(w["qkv"], w["qkv"].view(-1)[C:], b.rpb, w["att"], B=B, h=H, w=W, C_=C, heads=self.heads, ws=ws,
                                   ldq=3 * C, ldkv=3 * C, ldo=C, dtype=dt)
            self._lin(b.to_out, w["att"], xb, geo=geo, ldx=C, ldo=C, out_mode=O_NHWC_F32, r1=xa, ldr1=C)
            xa, xb = xb, xa
            if taps is not None and bi == 0:
                taps["attn0"] = xa.clone()
            for ci, (ln, ffn, esc) in enumerate(b.convs):
                self._convffn(ffn, xa, w["z"], **geo, dtype=dt, ln=ln, eps=LN_EPS, partials=w["gap"], ldx=C, ldo=C)
                self._lk_weights(esc, w, tiles, N, B)
                if esc.conv13:
                    ops.esc_conv13(w["z"], w["weff"], w["y16"], **geo, ldx=C, kpad=esc.kpad, dtype=dt)
                else:
                    pw = ops.PackedConv(w["weff"], esc.zero_bias, 13, 16, esc.kpad, 1, 1, 16, w_bstride=16 * esc.kpad)
                    ops.conv(pw, w["z"], w["y16"], **geo, dtype=dt, ldx=C, ldo=16, n_store=16)
                self._lin(esc.aggr, w["z"], xb, geo=geo, ldx=C, ldo=C, out_mode=O_NHWC_F32, x0=w["y16"], c_split=16, ldx0=16, r1=xa, ldr1=C)
                xa, xb = xb, xa
                if taps is not None and bi == 0 and ci == 0:
                    taps["conv0"] = xa.clone()
            self._layernorm(xa, w["n"], *b.ln_out, npix=B * N, dtype=dt, eps=LN_EPS, ldx=C, ldy=C)
            ops.conv(b.conv_out, w["n"], xb, **geo, dtype=dt, ldx=C, ldo=C, out_mode=O_NHWC_F32, r1=cur, ldr1=C)
            cur = xb
        return self._tail(x, w, cur, geo)

    def _check_frame(self, H: int, W: int):
        pass

    def _tail(self, x, w, cur, geo):
        """last (+ feat0), to_img, the pixel shuffle plus the base image                                       esc_arch.py:383-385"""
        C, dt = self.C, self.dtype
        B, H, W = geo["B"], geo["H"], geo["W"]
        ops.conv(self.last, cur, w["n"], **geo, dtype=dt, ldx=C, ldo=C, x_mode=X_NHWC_F32, r1=w["feat0"], ldr1=C)
        ld = w["rows"].shape[2]
        ops.conv(self.to_img, w["n"], w["rows"], **geo, dtype=dt, ldx=C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
        ops.esc_shuffle_add(w["rows"], x, w["y"], B=B, H=H, W=W, s=self.scale, ld=ld)
        return w["y"]


class ESCRealEngine(ESCEngine):
    """ESCReal (esc_real_arch.py:402-475): ESC's body with use_ln, then
        hat_escreal_skip (feat0 + skip(x))  ->  last (+ that)  ->  the head:
        default   to_img.1, to_img.4 folded to conv 64 -> 256 + PixelShuffle(2) (+ LeakyReLU 0.2), to_img.6 (+ LeakyReLU 0.2), to_img.8 -> planes
        DySample  one pointwise launch [offset | scope | end_conv per group]  ->  hat_dysample
    DESIGN.md §4.15.  The default head is x4 whatever upscaling_factor says (two hard-coded nearest x2 steps, as the reference)."""

    def _pack_head(self, sd):
        dt, dev = self.dtype, self.dev
        self.dysample = bool(self.cfg.get("use_dysample", False))
        self.skip = ops.pack_escreal_skip(sd, "skip", dt, dev)
        if self.dysample:
            s = self.scale
            if s not in (2, 3, 4):
                raise ValueError(f"ESCReal with use_dysample and upscaling_factor={s} is not supported: hat_dysample is built for 2, 3 and 4")
            f32 = lambda k: sd[k].detach().to(torch.float32).cpu()
            wd, bd = ops.dysample_fold(f32("to_img.offset.weight"), f32("to_img.offset.bias"), f32("to_img.scope.weight"),
                                       f32("to_img.end_conv.weight"))
            self.dys = ops.pack_pointwise(wd, bd, dt, dev)
            self.dys_ld = wd.shape[0]
            self.dys_init = f32("to_img.init_pos").reshape(-1).contiguous().to(dev)
            self.dys_bias = f32("to_img.end_conv.bias").contiguous().to(dev)
            self.out_scale = s
            return
        self.out_scale = 4
        self.up1 = ops.pack_nearest_conv(sd["to_img.1.weight"], sd["to_img.1.bias"], dt, dev)
        self.up2 = ops.pack_nearest_conv(sd["to_img.4.weight"], sd["to_img.4.bias"], dt, dev)
        self.hr = ops.pack_conv_weight(sd["to_img.6.weight"], sd["to_img.6.bias"], dt, dev)
        self.out = ops.pack_conv_weight(sd["to_img.8.weight"], sd["to_img.8.bias"], dt, dev)
        self.out_sweep = None   # the row-sweep kernel for the 64 -> 3 conv at output size, where HATEngine takes it for conv_last
        if ops.conv3x3_to_planes_supported(3, 64, 16, dt):
            self.out_sweep = ops.pack_cab_squeeze(sd["to_img.8.weight"], sd["to_img.8.bias"], dev)

    def _head_buffers(self, B, H, W, f, t):
        s = self.out_scale
        w = {"y": f(B, 3, H * s, W * s)}
        if self.dysample:
            w["rows"] = f(B, H * W, self.dys_ld)
        else:
            w.update(u1=t(B, 4 * H * W, 64), u2=t(B, 16 * H * W, 64), u3=t(B, 16 * H * W, 64))
        return w

    def _check_frame(self, H, W):
        if H < 4 or W < 4:
            raise RuntimeError(f"a {H}x{W} frame cannot be reflect-padded by 3 for the skip branch's 7x7 conv: a side of at least 4 is needed")

    def _tail(self, x, w, cur, geo):
        C, dt = self.C, self.dtype
        B, H, W = geo["B"], geo["H"], geo["W"]
        sk = next(s for s in w["s"] if s is not cur)
        ops.escreal_skip(self.skip, x, sk, **geo, dtype=dt, r=w["feat0"], ldr=C, ldo=C)
        ops.conv(self.last, cur, w["n"], **geo, dtype=dt, ldx=C, ldo=C, x_mode=X_NHWC_F32, r1=sk, ldr1=C)
        if self.dysample:
            self._lin(self.dys, w["n"], w["rows"], geo=geo, ldx=C, ldo=self.dys_ld, out_mode=O_NHWC_F32)
            ops.dysample(w["rows"], self.dys_init, self.dys_bias, w["y"], **geo, s=self.scale, ld=self.dys_ld)
            return w["y"]
        ops.conv(self.up1, w["n"], w["u1"], **geo, dtype=dt, ldx=C, ldo=C, out_mode=O_PIXSHUF_T, ps_r=2, act=ACT_LRELU02)
        ops.conv(self.up2, w["u1"], w["u2"], B=B, H=2 * H, W=2 * W, dtype=dt, ldx=C, ldo=C, out_mode=O_PIXSHUF_T, ps_r=2, act=ACT_LRELU02)
        ops.conv(self.hr, w["u2"], w["u3"], B=B, H=4 * H, W=4 * W, dtype=dt, ldx=C, ldo=C, act=ACT_LRELU02)
        if self.out_sweep is not None and (4 * W) % 16 == 0:
            wpk, b8 = self.out_sweep
            ops.conv3x3_to_planes(w["u3"], wpk, b8, w["y"], B=B, H=4 * H, W=4 * W, C_=C, ldx=C, n_out=3, out_scale=1.0, mean=(0.0, 0.0, 0.0, 0.0),
                                  dtype=dt)
        else:
            ops.conv(self.out, w["u3"], w["y"], B=B, H=4 * H, W=4 * W, dtype=dt, ldx=C, ldo=0, out_mode=O_NCHW_F32)
        return w["y"]


class ESCRealMEngine(ESCRealEngine):
    """ESCRealM (esc_real_arch.py:478-661): ESCReal's body and residual, with
        unshuffle mode   hat_unshuffle_pad (reflect pad + PixelUnshuffle(f) -> fp32 rows of 3 f^2 channels)  ->  proj on those rows,
                         hat_escrealm_skip in place of hat_escreal_skip; the body runs at ceil(h/f) x ceil(w/f), the head is x4 and the
                         output is the (s h, s w) corner of its buffer
        plain mode       ESCReal's stem
    and UniUpsample's five heads at the internal scale S (4 in unshuffle mode, else upscaling_factor):
        conv                 to_img.0 -> planes (the row-sweep kernel where it applies)
        pixelshuffledirect   to_img.0 -> fp32 rows, hat_shuffle_planes
        pixelshuffle         to_img.0 (+ LeakyReLU 0.01), one or two 3x3 mid -> r^2 mid with the pixel shuffle in the store, 3x3 mid -> 3
        nearest+conv         per step conv -> nearest x r -> LeakyReLU 0.2 as ONE conv 64 -> 64 r^2 (rows repeated) with the shuffle in
                             the store and the activation in the epilogue; then conv (+ LeakyReLU 0.2), conv -> planes
        dysample             [to_img.0 (+ LeakyReLU 0.01) when mid_dim != dim,] ESCReal's pointwise fold and hat_dysample
    DESIGN.md §4.18."""

    def _check_cfg(self, cfg):
        super()._check_cfg(cfg)
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

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        self.f = int(cfg["unshuffle"])
        if self.f:   # the plain-named keys the shared packing reads
            sd = dict(sd)
            sd["proj.weight"], sd["proj.bias"] = sd["proj.1.weight"], sd["proj.1.bias"]
        super().__init__(cfg, sd, device, compute_dtype)

    def _pack_head(self, sd):
        dt, dev, cfg = self.dtype, self.dev, self.cfg
        self.dysample = False   # (ESCRealEngine's flag; this class dispatches on self.head)
        self.skip = ops.pack_escrealm_skip(sd, "skip", dt, dev) if self.f else ops.pack_escreal_skip(sd, "skip", dt, dev)
        S = self.S = int(cfg["head_scale"])
        self.out_scale = S
        self.head = "conv" if S == 1 else cfg["upsampler"]
        mid = self.mid = int(cfg["mid_dim"])
        conv = lambda i: ops.pack_conv_weight(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], dt, dev)
        self.out_sweep = None
        if self.head == "conv":
            self.out_scale = 1
            self._pack_out(sd, 0)
        elif self.head == "pixelshuffledirect":
            self.direct = conv(0)
        elif self.head == "pixelshuffle":
            self.pre = conv(0)
            self.steps = [(2, 3)] if S == 3 else [(2 + 2 * k, 2) for k in range(S // 2)]   # (index in the Sequential, r)
            self.ups = [ops.pack_pixshuf_conv(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], r, dt, dev) for i, r in self.steps]
            self.out = conv(self.steps[-1][0] + 2)
        elif self.head == "nearest+conv":
            self.steps = [(0, 3)] if S == 3 else [(3 * k, 2) for k in range(S // 2)]
            self.ups = [ops.pack_conv_nearest(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], r, dt, dev) for i, r in self.steps]
            i = self.steps[-1][0] + 3
            self.hr = conv(i)
            self._pack_out(sd, i + 2)
        else:   # dysample
            p = "to_img.0"
            self.pre = None
            if mid != self.C:
                self.pre, p = conv(0), "to_img.2"
            f32 = lambda k: sd[k].detach().to(torch.float32).cpu()
            wd, bd = ops.dysample_fold(f32(p + ".offset.weight"), f32(p + ".offset.bias"), f32(p + ".scope.weight"), f32(p + ".end_conv.weight"))
            self.dys = ops.pack_pointwise(wd, bd, dt, dev)
            self.dys_ld = wd.shape[0]
            self.dys_init = f32(p + ".init_pos").reshape(-1).contiguous().to(dev)
            self.dys_bias = f32(p + ".end_conv.bias").contiguous().to(dev)

    def _pack_out(self, sd, i: int):
        """The 64 -> 3 conv into planes: hat_conv, and the row-sweep kernel where HATEngine takes it for conv_last."""
        self.out = ops.pack_conv_weight(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], self.dtype, self.dev)
        if ops.conv3x3_to_planes_supported(3, 64, 16, self.dtype):
            self.out_sweep = ops.pack_cab_squeeze(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], self.dev)

    def _body_size(self, h, w):
        f = self.f
        return (-(-h // f), -(-w // f)) if f else (h, w)

    def _alloc_workspace(self, B, h, w, tag=None):
        ws = super()._alloc_workspace(B, h, w, tag)
        if self.f:
            H, W = self._body_size(h, w)
            ws["xr"] = torch.zeros(B, H * W, 3 * self.f ** 2, dtype=torch.float32, device=self.dev)
        return ws

    def _head_buffers(self, B, H, W, f, t):
        S, N, hd = self.out_scale, H * W, self.head
        w = {"y": f(B, 3, H * S, W * S)}
        if hd == "pixelshuffledirect":
            w["rows"] = f(B, N, _r4(3 * S * S))
        elif hd in ("pixelshuffle", "nearest+conv"):
            ch, npx, w["u"] = (self.mid if hd == "pixelshuffle" else 64), N, []
            for _, r in self.steps:   # the map after each upsampling step
                npx *= r * r
                w["u"].append(t(B, npx, ch))
            if hd == "pixelshuffle":
                w["pre"] = t(B, N, ch)
            else:
                w["hr"] = t(B, npx, 64)
        elif hd == "dysample":
            if self.pre is not None:
                w["pre"] = t(B, N, self.mid)
            w["rows"] = f(B, N, self.dys_ld)
        return w

    def _check_frame(self, H, W):
        if H < 4 or W < 4:
            raise RuntimeError(f"a {H}x{W} map cannot be reflect-padded by 3 for the skip branch's 7x7 conv: a side of at least 4 is needed"
                               + (f" behind the /{self.f} unshuffle" if self.f else ""))

    def _stem(self, x, w, geo):
        if not self.f:
            return super()._stem(x, w, geo)
        B, _, h, wd = x.shape
        cin = 3 * self.f ** 2
        ops.unshuffle_pad(x, w["xr"], B=B, h=h, w=wd, f=self.f, ld=cin)
        ops.conv(self.proj, w["xr"], w["feat0"], **geo, dtype=self.dtype, ldx=cin, ldo=self.C, x_mode=X_NHWC_F32, out_mode=O_NHWC_F32)

    def _to_planes(self, src, y, B, H, W):
        C, dt = self.C, self.dtype
        if self.out_sweep is not None and self.out.cin == 64 and W % 16 == 0:
            wpk, b8 = self.out_sweep
            ops.conv3x3_to_planes(src, wpk, b8, y, B=B, H=H, W=W, C_=C, ldx=C, n_out=3, out_scale=1.0, mean=(0.0, 0.0, 0.0, 0.0), dtype=dt)
        else:
            ops.conv(self.out, src, y, B=B, H=H, W=W, dtype=dt, ldx=self.out.cin, ldo=0, out_mode=O_NCHW_F32)

    def _tail(self, x, w, cur, geo):
        C, dt, S, hd = self.C, self.dtype, self.out_scale, self.head
        B, H, W = geo["B"], geo["H"], geo["W"]
        sk = next(s for s in w["s"] if s is not cur)
        if self.f:
            ops.escrealm_skip(self.skip, w["xr"], sk, **geo, dtype=dt, ldx=w["xr"].shape[2], r=w["feat0"], ldr=C, ldo=C)
        else:
            ops.escreal_skip(self.skip, x, sk, **geo, dtype=dt, r=w["feat0"], ldr=C, ldo=C)
        ops.conv(self.last, cur, w["n"], **geo, dtype=dt, ldx=C, ldo=C, x_mode=X_NHWC_F32, r1=sk, ldr1=C)
        if hd == "conv":
            self._to_planes(w["n"], w["y"], B, H, W)
        elif hd == "pixelshuffledirect":
            ld = w["rows"].shape[2]
            ops.conv(self.direct, w["n"], w["rows"], **geo, dtype=dt, ldx=C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
            ops.shuffle_planes(w["rows"], w["y"], **geo, s=S, ld=ld)
        elif hd in ("pixelshuffle", "nearest+conv"):
            src, ch, hh, ww = w["n"], C, H, W
            if hd == "pixelshuffle":
                ch = self.mid
                ops.conv(self.pre, w["n"], w["pre"], **geo, dtype=dt, ldx=C, ldo=ch, act=ACT_LRELU)
                src = w["pre"]
            for (_, r), pw, u in zip(self.steps, self.ups, w["u"]):
                ops.conv(pw, src, u, B=B, H=hh, W=ww, dtype=dt, ldx=ch, ldo=ch, out_mode=O_PIXSHUF_T, ps_r=r,
                         act=ACT_LRELU02 if hd == "nearest+conv" else ops.ACT_NONE)
                src, hh, ww = u, hh * r, ww * r
            if hd == "nearest+conv":
                ops.conv(self.hr, src, w["hr"], B=B, H=hh, W=ww, dtype=dt, ldx=C, ldo=C, act=ACT_LRELU02)
                src = w["hr"]
            self._to_planes(src, w["y"], B, hh, ww)
        else:
            src, ch = w["n"], C
            if self.pre is not None:
                ch = self.mid
                ops.conv(self.pre, w["n"], w["pre"], **geo, dtype=dt, ldx=C, ldo=ch, act=ACT_LRELU)
                src = w["pre"]
            self._lin(self.dys, src, w["rows"], geo=geo, ldx=ch, ldo=self.dys_ld, out_mode=O_NHWC_F32)
            ops.dysample(w["rows"], self.dys_init, self.dys_bias, w["y"], **geo, s=S, ld=self.dys_ld)
        if self.f:   # the reference's crop to (s h, s w): a corner of the x4 buffer
            s = self.scale
            return w["y"][:, :, :s * x.shape[2], :s * x.shape[3]]
        return w["y"]


FP_SUPPORTED = dict(dim=48, pdim=16, kernel_size=13, window_size=32, num_heads=3)


class ESCFPEngine(ESCEngine):
    """ESCFP (esc_fp_arch.py:277-355): ESC's Block loop at 48 channels and 3 heads, with a LayerNorm in front of every conv block,
    hat_escfp_weights in place of hat_esc_weights (the decomposed large-kernel branch folded to the dense rank-1 filter the 13x13
    conv kernels read), then
        hat_escfp_layernorm (ln_last)  ->  last (+ feat0)  ->  to_img  ->  hat_escfp_shuffle_bicubic
    Batches are taken: workspace, pool partials and weight images are per sample.  DESIGN.md §4.16."""

    _convffn, _layernorm, _pack_ffn = staticmethod(ops.escfp_convffn), staticmethod(ops.escfp_layernorm), staticmethod(ops.pack_escfp_convffn)

    def _check_cfg(self, cfg):
        for k, v in FP_SUPPORTED.items():
            if int(cfg[k]) != v:
                raise ValueError(f"ESCFP with {k}={cfg[k]} is not supported: the device path is built for "
                                 + ", ".join(f"{a}={b}" for a, b in FP_SUPPORTED.items()) + " (ESC_FP_X2 / X3 / X4)")
        if int(cfg["dim"] * cfg["exp_ratio"]) not in ops.ESCFP_HID_PAD:
            raise ValueError(f"ESCFP with exp_ratio={cfg['exp_ratio']} is not supported: hat_escfp_convffn is built for a hidden width of "
                             + ", ".join(map(str, ops.ESCFP_HID_PAD)) + " (exp_ratio 1.25, 1.5, 2)")
        if int(cfg["upscaling_factor"]) not in (2, 3, 4):
            raise ValueError(f"ESCFP with upscaling_factor={cfg['upscaling_factor']} is not supported: hat_escfp_shuffle_bicubic is built for 2, 3 and 4")

    def _shared_filter(self, sd):
        return sd   # lk_channel / lk_spatial are used as they are: no geometric ensemble, no convert()

    def _pack_lk(self, sd, core: str):
        return ops.pack_escfp_lk(sd, core, self.dtype, self.dev)

    def _lk_weights(self, esc, w, tiles, N, B):
        ops.escfp_weights(w["gap"], tiles, N, esc, w["weff"], B=B, dtype=self.dtype)

    def _check_batch(self, B):
        pass

    def _pack_head(self, sd):
        super()._pack_head(sd)
        vec = lambda k: sd[k].detach().to(dtype=torch.float32, device=self.dev).contiguous()
        self.ln_last = (vec("ln_last.weight"), vec("ln_last.bias"))
        self.ptab = ops.bicubic_phase_table(self.scale).to(self.dev)

    def _tail(self, x, w, cur, geo):
        """ln_last, last (+ feat0), to_img, the pixel shuffle plus the bicubic base image                   esc_fp_arch.py:352-354"""
        C, dt = self.C, self.dtype
        B, H, W = geo["B"], geo["H"], geo["W"]
        self._layernorm(cur, w["z"], *self.ln_last, npix=B * H * W, dtype=dt, eps=LN_EPS, ldx=C, ldy=C)
        ops.conv(self.last, w["z"], w["n"], **geo, dtype=dt, ldx=C, ldo=C, r1=w["feat0"], ldr1=C)
        ld = w["rows"].shape[2]
        ops.conv(self.to_img, w["n"], w["rows"], **geo, dtype=dt, ldx=C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
        ops.escfp_shuffle_bicubic(w["rows"], x, self.ptab, w["y"], B=B, H=H, W=W, s=self.scale, ld=ld)
        return w["y"]


class ESCLTEEngine(ESCEngine):
    """ESC-LTE (esc_arb/models/lte.py, esc.py): ESC's Block loop as the encoder (no to_img; the geometric filter ensemble on every
    forward), then
        last (+ feat0)  ->  hat_conv 64 -> 512 (coef | freq, fp32 rows)         gen_feat, kept in the workspace of the shape
        hat_lte_query                                                           query / query_grid, any number of times
    The state dict is the reference LTE's: the encoder's keys under `encoder.`, the head's beside them.  DESIGN.md §4.19."""

    def __init__(self, cfg, sd, device, compute_dtype="bf16"):
        sd = dict(sd)
        for k in [k for k in sd if k.startswith("encoder.")]:   # the plain-named keys the shared packing reads
            sd[k[len("encoder."):]] = sd[k]
        self._feat_ws = None
        super().__init__(dict(cfg, upscaling_factor=1), sd, device, compute_dtype)

    def _check_cfg(self, cfg):
        super()._check_cfg(cfg)
        hd, hl = int(cfg.get("hidden_dim", 256)), tuple(int(v) for v in cfg.get("hidden_list", (256, 256, 256)))
        if hd != ops.LTE_HIDDEN or hl != (ops.LTE_HIDDEN,) * 3:
            raise ValueError(f"ESC-LTE with hidden_dim={hd}, hidden_list={hl} is not supported: hat_lte_query is built for hidden_dim "
                             f"{ops.LTE_HIDDEN} and hidden_list {(ops.LTE_HIDDEN,) * 3}")

    def _pack_head(self, sd):
        self.lte = ops.pack_lte(sd, self.dtype, self.dev)

    def _head_buffers(self, B, H, W, f, t):
        return {"cf": f(B, H * W, 2 * ops.LTE_HIDDEN), "x": f(B, 3, H, W)}

    def _tail(self, x, w, cur, geo):
        """last (+ feat0); coef | freq as one 512-wide conv into fp32 rows; the input kept for the bilinear base      lte.py:23-32"""
        C, dt = self.C, self.dtype
        ops.conv(self.last, cur, w["n"], **geo, dtype=dt, ldx=C, ldo=C, x_mode=X_NHWC_F32, r1=w["feat0"], ldr1=C)
        ld = w["cf"].shape[2]
        ops.conv(self.lte.taps, w["n"], w["cf"], **geo, dtype=dt, ldx=C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
        w["x"].copy_(x)
        self._feat_ws = (w, geo["H"], geo["W"])
        return w["n"]

    def _query(self, out, **kw):
        if self._feat_ws is None:
            raise RuntimeError("ESC-LTE: query before gen_feat: there are no features to query")
        w, H, W = self._feat_ws
        hd = ops.LTE_HIDDEN
        with self._lock, torch.cuda.device(self.dev):
            ops.lte_query(self.lte, w["cf"], w["cf"].view(-1)[hd:], w["x"], out, H=H, W=W, ldc=2 * hd, ldf=2 * hd, dtype=self.dtype, **kw)
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
    def _ws_f32(self, H: int, W: int, key: str, shape) -> torch.Tensor:
        """An fp32 buffer in the workspace of the (1, H, W) frame shape, allocated with its first use (FrameBoundary._ws_buffer's rule)."""
        ws = self._workspace(1, H, W)
        t = ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = ws[key] = torch.zeros(shape, dtype=torch.float32, device=self.dev)
            ws["bytes"] += t.numel() * 4
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

    def _query_sink(self, fn, *dst, **kw):
        if self._feat_ws is None:
            raise RuntimeError("ESC-LTE: query before gen_feat: there are no features to query")
        w, H, W = self._feat_ws
        hd = ops.LTE_HIDDEN
        with self._lock, torch.cuda.device(self.dev):
            fn(self.lte, w["cf"], w["cf"].view(-1)[hd:], w["x"], *dst, H=H, W=W, ldc=2 * hd, ldf=2 * hd, dtype=self.dtype, **kw)

    def query_grid_planes(self, out: torch.Tensor, cell_yx, out_affine=(1.0, 0.0)) -> torch.Tensor:
        """query_grid into the caller's (3,h,w) or (1,3,h,w) contiguous fp32 tensor."""
        return self._query(out, grid=tuple(out.shape[-2:]), cell_yx=cell_yx, out_affine=out_affine)

    def query_grid_u8(self, out: torch.Tensor, cell_yx, bgr: bool = False, out_affine=(0.5, 0.5)) -> torch.Tensor:
        """The grid of out's (h, w) -> out (1,h,w,3) uint8 (rows may be pitched): tensor2img's bytes of the image * a + b."""
        self._query_sink(ops.lte_query_u8, out, grid=tuple(out.shape[-3:-1]), cell_yx=cell_yx, out_affine=out_affine, bgr=bgr)
        return out

    def query_grid_yuv(self, out_views, cell_yx, from_rgb, sub, depth: int = 8, msb=False, out_affine=(0.5, 0.5)) -> None:
        """The grid of the Y view's (h, w) -> the views (y, cb, cr) of a centre-sited frame (ops.yuv_views) of the image * a + b."""
        y, cb, cr = out_views
        self._query_sink(ops.lte_query_yuv, y, cb, cr, from_rgb, grid=tuple(y.shape[-2:]), cell_yx=cell_yx, out_affine=out_affine, sub=sub,
                         depth=depth, msb=msb)
