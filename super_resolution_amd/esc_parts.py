"""The parts an `ESCEngine` (esc_engine.py) is put together from.  The networks of the ESC family share the Block loop and differ in
    the stem       how feat0 is made from the frame
    the residual   what `last` adds: feat0, or feat0 + skip(x)
    the head       `last`, and how its 64- or 48-channel map becomes an image
A part is made as Part(engine, sd, **options) and has three duties: `pack(sd)` at construction, `buffers(B, H, W, f, t)` -> the
tensors (or lists of tensors) it adds to the workspace of a shape (a FLAT dict: EngineBase._workspace sums top-level entries into
w["bytes"]; H, W are the body's size, f / t allocate fp32 / T tensors), and `run`, its launches.  DESIGN.md §4.14-§4.19 have the
launch lists."""
from __future__ import annotations

import torch

from . import ops
from .ops import ACT_LRELU, ACT_LRELU02, ACT_NONE, O_NCHW_F32, O_NHWC_F32, O_PIXSHUF_T, X_NCHW_F32_MEAN, X_NHWC_F32, X_NHWC_T

LN_EPS = 1e-6   # esc_arch.py:69


def _r4(n: int) -> int:
    return (n + 3) // 4 * 4


def _f32(sd, k):
    return sd[k].detach().to(torch.float32).cpu()


class Part:
    def __init__(self, e, sd, **options):
        self.e = e   # the engine: dev, dtype, C, scale, cfg, _lin
        self.__dict__.update(options)
        self.pack(sd)

    def pack(self, sd):
        pass

    def buffers(self, B, H, W, f, t) -> dict:
        return {}

    def conv(self, sd, name: str):
        return ops.pack_conv_weight(sd[name + ".weight"], sd[name + ".bias"], self.e.dtype, self.e.dev)


# ---- stems: run(x, w, geo) writes w["feat0"] ----------------------------------------------------------------------------------
class PlainStem(Part):
    """feat0 = proj(x - mean) on the NCHW frame"""
    f = 0   # no unshuffle: the body runs at the frame's size

    def pack(self, sd):
        self.proj = self.conv(sd, "proj")

    def body_size(self, h: int, w: int):
        """The size the body runs at for an (h, w) frame."""
        return h, w

    def run(self, x, w, geo):
        e = self.e
        ops.conv(self.proj, x, w["feat0"], **geo, dtype=e.dtype, ldx=0, ldo=e.C, x_mode=X_NCHW_F32_MEAN, out_mode=O_NHWC_F32)


class UnshuffledStem(Part):
    """ESCRealM's (option f): hat_unshuffle_pad (reflect pad to a multiple of f + PixelUnshuffle(f) -> fp32 rows of 3 f^2 channels,
    kept in w["xr"] for the skip branch), then proj on those rows.  The body runs at ceil(h/f) x ceil(w/f)."""

    def pack(self, sd):
        self.proj = self.conv(sd, "proj.1")

    def body_size(self, h, w):
        return -(-h // self.f), -(-w // self.f)

    def buffers(self, B, H, W, f, t):
        return {"xr": f(B, H * W, 3 * self.f ** 2)}

    def run(self, x, w, geo):
        e, cin = self.e, 3 * self.f ** 2
        ops.unshuffle_pad(x, w["xr"], B=x.shape[0], h=x.shape[2], w=x.shape[3], f=self.f, ld=cin)
        ops.conv(self.proj, w["xr"], w["feat0"], **geo, dtype=e.dtype, ldx=cin, ldo=e.C, x_mode=X_NHWC_F32, out_mode=O_NHWC_F32)


# ---- residuals: run(x, w, cur, geo) -> the fp32 rows `last` adds ---------------------------------------------------------------
class Feat0Residual(Part):
    def check_frame(self, H: int, W: int):
        pass

    def run(self, x, w, cur, geo):
        return w["feat0"]


class SkipResidual(Part):
    """feat0 + skip(x), hat_escreal_skip (the reflect-padded 7x7 branch on the frame), into a stream buffer that is not `cur`: the
    body is done with the other two.  Options: what ("frame" / "map") and behind, the words of the frame check."""
    behind = ""

    def pack(self, sd):
        self.skip = ops.pack_escreal_skip(sd, "skip", self.e.dtype, self.e.dev)

    def check_frame(self, H, W):
        if H < 4 or W < 4:
            raise RuntimeError(f"a {H}x{W} {self.what} cannot be reflect-padded by 3 for the skip branch's 7x7 conv: a side of at least 4 "
                               "is needed" + self.behind)

    def run(self, x, w, cur, geo):
        sk = next(s for s in w["s"] if s is not cur)
        self.launch(x, w, sk, geo)
        return sk

    def launch(self, x, w, sk, geo):
        ops.escreal_skip(self.skip, x, sk, **geo, dtype=self.e.dtype, r=w["feat0"], ldr=self.e.C, ldo=self.e.C)


class UnshuffledSkipResidual(SkipResidual):
    """The same on the unshuffled rows the stem left in w["xr"]: hat_escrealm_skip."""

    def pack(self, sd):
        self.skip = ops.pack_escrealm_skip(sd, "skip", self.e.dtype, self.e.dev)

    def launch(self, x, w, sk, geo):
        ops.escrealm_skip(self.skip, w["xr"], sk, **geo, dtype=self.e.dtype, ldx=w["xr"].shape[2], r=w["feat0"], ldr=self.e.C, ldo=self.e.C)


# ---- heads: run(x, w, cur, res, geo, sink=None) -> the forward's result: the planes w["y"], or with a sink (frame_boundary._Sink)
# sink.out, filled by one of three routes: the conv route (ToPlanes: the row sweep's byte / YCbCr epilogue, else planes), the
# shuffle route (hat_shuffle_to_u8 / hat_shuffle_to_yuv where the sink is fusable, else planes), planes only (Head.end) -----------
class ToPlanes:
    """A 3x3 conv to 3 channels stored as fp32 NCHW planes: hat_conv, or (sweep=True) the row-sweep kernel where HATEngine takes it
    for conv_last: 64 input channels, T rows it is built for, a width that is a multiple of 16.
    The call sites this replaces asked, with W the BODY's width at the first and the conv's own at the second,
        ESCReal's default head    out_sweep is not None and (4 * W) % 16 == 0        the conv runs at width 4 W: the same number
        ESCRealM's heads          out_sweep is not None and out.cin == 64 and W % 16 == 0
    and out_sweep was packed for the "conv" and "nearest+conv" heads only, whose last conv reads C = 64 channels (the engines
    refuse any other dim), so `cin == 64` held wherever out_sweep was not None.  "pixelshuffle" never packed it, also at mid_dim
    64: it passes sweep=False."""

    def __init__(self, part, sd, name: str, sweep: bool = True):
        self.e, self.out, self.sweep = part.e, part.conv(sd, name), None
        if sweep and ops.conv3x3_to_planes_supported(3, 64, 16, self.e.dtype):
            self.sweep = ops.pack_cab_squeeze(sd[name + ".weight"], sd[name + ".bias"], self.e.dev)

    def run(self, src, y, B, H, W, sink=None):
        """H, W: the size the conv runs at.  With a sink the row sweep converts in its epilogue where it runs and the sink can take
        it (hat_conv3x3_to_u8 / hat_conv3x3_to_yuv; y is not written); else the planes y are written as always and the sink
        converts them.  -> the result: y, or sink.out."""
        C, dt = self.out.cin, self.e.dtype
        if sink is not None and self.sweep is not None and W % 16 == 0 and sink.fusable:
            sink.fused(src, *self.sweep, B=B, H=H, W=W, C_=C, ldx=C, out_scale=1.0, mean=(0.0, 0.0, 0.0, 0.0), dtype=dt)
            return sink.out
        if self.sweep is not None and W % 16 == 0:
            ops.conv3x3_to_planes(src, *self.sweep, y, B=B, H=H, W=W, C_=C, ldx=C, n_out=3, out_scale=1.0, mean=(0.0, 0.0, 0.0, 0.0), dtype=dt)
        else:
            ops.conv(self.out, src, y, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=0, out_mode=O_NCHW_F32)
        return Head.end(y, sink)


class Head(Part):
    out_scale = None   # the factor between the body's size and w["y"]'s, where it is not the engine's scale

    def last(self, w, src, res, geo, x_mode=X_NHWC_F32):
        """n = last(src) + res"""
        e = self.e
        ops.conv(e.last, src, w["n"], **geo, dtype=e.dtype, ldx=e.C, ldo=e.C, x_mode=x_mode, r1=res, ldr1=e.C)

    def y(self, B, H, W, f):
        s = self.out_scale or self.e.scale
        return f(B, 3, H * s, W * s)

    @staticmethod
    def end(y, sink):
        """The result of a head that wrote the planes y: y itself, or the sink's, converted from them (the sink's size is the crop)."""
        if sink is None:
            return y
        sink.from_planes(y)
        return sink.out

    def rows_conv(self, pw, w, geo):
        """A conv from n into all of the fp32 rows w["rows"] -> their width."""
        ld = w["rows"].shape[2]
        ops.conv(pw, w["n"], w["rows"], **geo, dtype=self.e.dtype, ldx=self.e.C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
        return ld


class ShuffleAddHead(Head):
    """ESC: last (+ res), to_img, the pixel shuffle plus the base image                                    esc_arch.py:383-385"""

    def pack(self, sd):
        self.to_img = self.conv(sd, "to_img")

    def buffers(self, B, H, W, f, t):
        return {"rows": f(B, H * W, _r4(3 * self.e.scale ** 2)), "y": self.y(B, H, W, f)}

    def run(self, x, w, cur, res, geo, sink=None):
        self.last(w, cur, res, geo)
        ld = self.rows_conv(self.to_img, w, geo)
        if sink is not None and sink.fusable:   # rows + base image straight to the frame: w["y"] is not written
            sink.shuffled(w["rows"], x, **geo, s=self.e.scale, ld=ld)
            return sink.out
        ops.esc_shuffle_add(w["rows"], x, w["y"], **geo, s=self.e.scale, ld=ld)
        return self.end(w["y"], sink)


class ShuffleBicubicHead(ShuffleAddHead):
    """ESCFP: ln_last into z, last from THERE (+ res), to_img, the pixel shuffle plus the bicubic base image   esc_fp_arch.py:352-354"""

    def pack(self, sd):
        super().pack(sd)
        self.ln_last = tuple(sd[k].detach().to(dtype=torch.float32, device=self.e.dev).contiguous() for k in ("ln_last.weight", "ln_last.bias"))
        self.ptab = ops.bicubic_phase_table(self.e.scale).to(self.e.dev)

    def run(self, x, w, cur, res, geo, sink=None):   # (a sink always converts the planes: DESIGN.md §4.21)
        e = self.e
        e.width.layernorm(cur, w["z"], *self.ln_last, npix=geo["B"] * geo["H"] * geo["W"], dtype=e.dtype, eps=LN_EPS, ldx=e.C, ldy=e.C)
        self.last(w, w["z"], res, geo, x_mode=X_NHWC_T)
        ld = self.rows_conv(self.to_img, w, geo)
        ops.escfp_shuffle_bicubic(w["rows"], x, self.ptab, w["y"], **geo, s=e.scale, ld=ld)
        return self.end(w["y"], sink)


class NearestX4Head(Head):
    """ESCReal's default head, x4 whatever upscaling_factor says (two hard-coded nearest x2 steps, as the reference): to_img.1 and
    to_img.4 folded to conv 64 -> 256 + PixelShuffle(2) (+ LeakyReLU 0.2), to_img.6 (+ LeakyReLU 0.2), to_img.8 -> planes."""
    out_scale = 4

    def pack(self, sd):
        e = self.e
        self.ups = [ops.pack_nearest_conv(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], e.dtype, e.dev) for i in (1, 4)]
        self.hr, self.out = self.conv(sd, "to_img.6"), ToPlanes(self, sd, "to_img.8")

    def buffers(self, B, H, W, f, t):
        return {"y": self.y(B, H, W, f), "u1": t(B, 4 * H * W, 64), "u2": t(B, 16 * H * W, 64), "u3": t(B, 16 * H * W, 64)}

    def run(self, x, w, cur, res, geo, sink=None):
        C, dt = self.e.C, self.e.dtype
        B, H, W = geo["B"], geo["H"], geo["W"]
        self.last(w, cur, res, geo)
        ops.conv(self.ups[0], w["n"], w["u1"], **geo, dtype=dt, ldx=C, ldo=C, out_mode=O_PIXSHUF_T, ps_r=2, act=ACT_LRELU02)
        ops.conv(self.ups[1], w["u1"], w["u2"], B=B, H=2 * H, W=2 * W, dtype=dt, ldx=C, ldo=C, out_mode=O_PIXSHUF_T, ps_r=2, act=ACT_LRELU02)
        ops.conv(self.hr, w["u2"], w["u3"], B=B, H=4 * H, W=4 * W, dtype=dt, ldx=C, ldo=C, act=ACT_LRELU02)
        return self.out.run(w["u3"], w["y"], B, 4 * H, 4 * W, sink)


class DySampleHead(Head):
    """ESCReal's and ESCRealM's: [to_img.0 (+ LeakyReLU 0.01) to mid channels when pre,] one pointwise launch [offset | scope |
    end_conv per group], hat_dysample.  Options: out_scale, at (the DySample module's key), pre (False, or the width mid)."""

    def pack(self, sd):
        e, p = self.e, self.at
        self.pre_conv = self.conv(sd, "to_img.0") if self.pre else None
        wd, bd = ops.dysample_fold(_f32(sd, p + ".offset.weight"), _f32(sd, p + ".offset.bias"), _f32(sd, p + ".scope.weight"),
                                   _f32(sd, p + ".end_conv.weight"))
        self.dys, self.ld = ops.pack_pointwise(wd, bd, e.dtype, e.dev), wd.shape[0]
        self.init = _f32(sd, p + ".init_pos").reshape(-1).contiguous().to(e.dev)
        self.bias = _f32(sd, p + ".end_conv.bias").contiguous().to(e.dev)

    def buffers(self, B, H, W, f, t):
        w = {"y": self.y(B, H, W, f), "rows": f(B, H * W, self.ld)}
        if self.pre:
            w["pre"] = t(B, H * W, self.pre)
        return w

    def run(self, x, w, cur, res, geo, sink=None):   # (a sink always converts the planes: DESIGN.md §4.21)
        e = self.e
        self.last(w, cur, res, geo)
        src, ch = w["n"], e.C
        if self.pre:
            src, ch = w["pre"], self.pre
            ops.conv(self.pre_conv, w["n"], src, **geo, dtype=e.dtype, ldx=e.C, ldo=ch, act=ACT_LRELU)
        e._lin(self.dys, src, w["rows"], geo=geo, ldx=ch, ldo=self.ld, out_mode=O_NHWC_F32)
        ops.dysample(w["rows"], self.init, self.bias, w["y"], **geo, s=self.out_scale, ld=self.ld)
        return self.end(w["y"], sink)


class ConvHead(Head):
    """ESCRealM "conv" (and any upsampler at scale 1): to_img.0 -> planes, no upsampling"""
    out_scale = 1

    def pack(self, sd):
        self.out = ToPlanes(self, sd, "to_img.0")

    def buffers(self, B, H, W, f, t):
        return {"y": self.y(B, H, W, f)}

    def run(self, x, w, cur, res, geo, sink=None):
        self.last(w, cur, res, geo)
        return self.out.run(w["n"], w["y"], **geo, sink=sink)


class ShufflePlanesHead(Head):
    """ESCRealM "pixelshuffledirect" (option out_scale): to_img.0 -> fp32 rows, hat_shuffle_planes"""

    def pack(self, sd):
        self.direct = self.conv(sd, "to_img.0")

    def buffers(self, B, H, W, f, t):
        return {"y": self.y(B, H, W, f), "rows": f(B, H * W, _r4(3 * self.out_scale ** 2))}

    def run(self, x, w, cur, res, geo, sink=None):
        self.last(w, cur, res, geo)
        ld = self.rows_conv(self.direct, w, geo)
        if sink is not None and sink.fusable:   # rows straight to the frame: w["y"] is not written
            sink.shuffled(w["rows"], None, **geo, s=self.out_scale, ld=ld)
            return sink.out
        ops.shuffle_planes(w["rows"], w["y"], **geo, s=self.out_scale, ld=ld)
        return self.end(w["y"], sink)


class StepsHead(Head):
    """ESCRealM's two heads that upsample in steps of r (one r=3 step, or log2(S) r=2 steps), the shuffle in each step's store.
    Options: out_scale = S, nearest, mid.
        "pixelshuffle" (nearest=False)   to_img.0 (+ LeakyReLU 0.01) to mid channels, per step 3x3 mid -> r^2 mid, then 3x3 mid -> 3
        "nearest+conv" (nearest=True)    per step conv -> nearest x r -> LeakyReLU 0.2 as ONE conv 64 -> 64 r^2 (rows repeated) with
                                         the activation in the epilogue; then conv (+ LeakyReLU 0.2), conv -> planes"""

    def pack(self, sd):
        e, S = self.e, self.out_scale
        first, stride, fold = (0, 3, ops.pack_conv_nearest) if self.nearest else (2, 2, ops.pack_pixshuf_conv)   # indices in the Sequential
        self.steps = [(first, 3)] if S == 3 else [(first + stride * k, 2) for k in range(S // 2)]
        self.ups = [fold(sd[f"to_img.{i}.weight"], sd[f"to_img.{i}.bias"], r, e.dtype, e.dev) for i, r in self.steps]
        i = self.steps[-1][0] + stride
        self.ch = e.C if self.nearest else self.mid
        self.ends = self.conv(sd, f"to_img.{i}" if self.nearest else "to_img.0")   # nearest: after the steps; else: before them
        self.out = ToPlanes(self, sd, f"to_img.{i + 2}" if self.nearest else f"to_img.{i}", sweep=self.nearest)

    def buffers(self, B, H, W, f, t):
        w, npx = {"y": self.y(B, H, W, f), "u": []}, H * W
        for _, r in self.steps:   # the map after each upsampling step
            npx *= r * r
            w["u"].append(t(B, npx, self.ch))
        if self.nearest:
            w["hr"] = t(B, npx, 64)
        else:
            w["pre"] = t(B, H * W, self.ch)
        return w

    def run(self, x, w, cur, res, geo, sink=None):
        C, dt, ch = self.e.C, self.e.dtype, self.ch
        B, hh, ww = geo["B"], geo["H"], geo["W"]
        self.last(w, cur, res, geo)
        src = w["n"]
        if not self.nearest:
            ops.conv(self.ends, w["n"], w["pre"], **geo, dtype=dt, ldx=C, ldo=ch, act=ACT_LRELU)
            src = w["pre"]
        for (_, r), pw, u in zip(self.steps, self.ups, w["u"]):
            ops.conv(pw, src, u, B=B, H=hh, W=ww, dtype=dt, ldx=ch, ldo=ch, out_mode=O_PIXSHUF_T, ps_r=r, act=ACT_LRELU02 if self.nearest else ACT_NONE)
            src, hh, ww = u, hh * r, ww * r
        if self.nearest:
            ops.conv(self.ends, src, w["hr"], B=B, H=hh, W=ww, dtype=dt, ldx=C, ldo=C, act=ACT_LRELU02)
            src = w["hr"]
        return self.out.run(src, w["y"], B, hh, ww, sink)


class LTEHead(Head):
    """ESC-LTE: last (+ res); coef | freq as one 512-wide conv into fp32 rows; the input kept for the bilinear base  lte.py:23-32.
    What a query needs, (w, H, W), is left in the engine's _feat_ws; the forward returns the rows n."""

    def pack(self, sd):
        self.lte = ops.pack_lte(sd, self.e.dtype, self.e.dev)

    def buffers(self, B, H, W, f, t):
        return {"cf": f(B, H * W, 2 * ops.LTE_HIDDEN), "x": f(B, 3, H, W)}

    def run(self, x, w, cur, res, geo, sink=None):
        self.last(w, cur, res, geo)
        ld = w["cf"].shape[2]
        ops.conv(self.lte.taps, w["n"], w["cf"], **geo, dtype=self.e.dtype, ldx=self.e.C, ldo=ld, out_mode=O_NHWC_F32, n_store=ld)
        w["x"].copy_(x)
        self.e._feat_ws = (w, geo["H"], geo["W"])
        return w["n"]
