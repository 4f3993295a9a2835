"""`FrameBoundary` — where a forward starts or ends in something other than fp32 planes: the geometric self-ensemble and the byte,
ground-truth and YCbCr frame entry points, with the sinks (`_Sink`) a byte forward ends in.  It knows no network: an engine mixes it in."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


class _Sink:
    """Where a byte-frame forward ends instead of in fp32 planes: `out`, the caller's result tensor of the (h_out, w_out) top-left
    pixels, and the ways to fill it — fused(src, wpk, b8, conv_last's geometry ...), conv_last's row sweep with the conversion
    as its epilogue (no fp32 image exists); folded(src, pf, the folded ending's geometry ...), the same for hat_upfold_*; shuffled(rows, base, B, H, W, s, ld), the same for a head that ends in a pixel shuffle of
    fp32 rows (hat_shuffle_to_u8 / hat_shuffle_to_yuv; base: the image added, or None); or from_planes(y) of an fp32 image, which
    may be larger than `out`: the sink's size is the crop.  Each bumps its engine counter, `kind`_fused_calls or `kind`_planes_calls.  band_refusal: why a row band, which hands its rows over as fp32, cannot end in this sink."""
    kind = band_refusal = None
    fusable = True   # False: neither conv_last nor the shuffle has an epilogue for this sink; it always ends in from_planes

    def __init__(self, eng, out, size):
        self.eng, self.out, self.size = eng, out, size

    def _count(self, how):
        name = f"{self.kind}_{how}_calls"
        setattr(self.eng, name, getattr(self.eng, name) + 1)


class _U8Sink(_Sink):
    """out (B,h_out,w_out,3) uint8 by tensor2img's conversion: hat_conv3x3_to_u8 / hat_planes_to_u8."""
    kind, band_refusal = "u8", "a row band hands its rows over as fp32: the 8-bit output is the unsharded forward's"

    def __init__(self, eng, out, bgr):
        super().__init__(eng, out, tuple(out.shape[1:3]))
        self.bgr = bool(bgr)

    def fused(self, src, wpk, b8, **conv):
        ops.conv3x3_to_u8(src, wpk, b8, self.out, h_out=self.size[0], w_out=self.size[1], bgr=self.bgr, **conv)
        self._count("fused")

    def folded(self, src, pf, **conv):
        ops.upfold_to_u8(src, pf, self.out, h_out=self.size[0], w_out=self.size[1], bgr=self.bgr, **conv)
        self._count("fused")

    def shuffled(self, rows, base, **geo):
        ops.shuffle_to_u8(rows, base, self.out, bgr=self.bgr, **geo)
        self._count("fused")

    def from_planes(self, y):
        ops.planes_to_u8(y, self.out, bgr=self.bgr)
        self._count("planes")


class _YuvSink(_Sink):
    """out in a layout of yuv.LAYOUTS as its (y, cb, cr) views (ops.yuv_views; sub = (sub_x, sub_y), None: grey), `depth` bits a
    sample: hat_conv3x3_to_yuv / hat_planes_to_yuv, for the 4:2:0 layouts as for every other.  siting: the output's chroma siting
    (yuv.SITINGS).  Where the layout leaves an axis co-sited the sink is not fusable — conv_last's epilogue has no halo column or
    row — and ends in hat_planes_to_yuv_sited; every other siting is the centre sink."""
    kind, band_refusal = "yuv", "the 4:2:0 output is the unsharded forward's, and it is one target of three"

    def __init__(self, eng, out, views, from_rgb, *, sub, depth, msb, siting="center"):
        super().__init__(eng, out, tuple(views[0].shape[1:3]))
        self.views, self.from_rgb, self.surface = views, from_rgb, dict(sub=sub, depth=depth, msb=msb)
        self.siting = ops._siting(sub, siting)[0]
        self.fusable = self.siting == "center"

    def fused(self, src, wpk, b8, **conv):
        ops.conv3x3_to_yuv(src, wpk, b8, *self.views, from_rgb=self.from_rgb, **self.surface, **conv)
        self._count("fused")

    def folded(self, src, pf, **conv):
        ops.upfold_to_yuv(src, pf, *self.views, from_rgb=self.from_rgb, **self.surface, **conv)
        self._count("fused")

    def shuffled(self, rows, base, **geo):
        ops.shuffle_to_yuv(rows, base, *self.views, self.from_rgb, **self.surface, **geo)
        self._count("fused")

    def from_planes(self, y):
        ops.planes_to_yuv(y, *self.views, self.from_rgb, siting=self.siting, **self.surface)
        self._count("planes")


class _PackedSink(_Sink):
    """out in a packed 4:2:2 layout of yuv.PACKED_FORMATS (side: its ops.FrameSide).  No kernel that ends a network has a packed
    epilogue, so the sink is never fusable: it ends in fp32 planes and hat_planes_to_packed422, and counts under yuv_planes_calls."""
    kind, band_refusal, fusable = "yuv", _YuvSink.band_refusal, False

    def __init__(self, eng, out, side, from_rgb, width):
        super().__init__(eng, out, (out.shape[1], width))
        self.side, self.from_rgb, self.width = side, from_rgb, width

    def from_planes(self, y):
        self.side.from_planes(y, self.out, self.from_rgb, width=self.width)
        self._count("planes")


def yuv_sink(eng, out, side, from_rgb, width):
    """The sink of a YCbCr result `out` (already checked: side.out) whose layout, depth and siting are the ops.FrameSide `side`;
    width: the result's width in pixels (a v210 array does not give it)."""
    if side.packed:
        return _PackedSink(eng, out, side, from_rgb, width)
    return _YuvSink(eng, out, side.views(out), from_rgb, sub=side.sub, depth=side.depth, msb=side.msb, siting=side.siting)


class FrameBoundary:
    """Requires of its host engine: `_forward(x, one_stream=, sink=)` and `_check_input(x)`; `_workspace`, `scale`, `ws`, `dev`,
    `_lock` and `cfg["in_chans"]`; and the four counters `u8_fused_calls`, `u8_planes_calls`, `yuv_fused_calls`, `yuv_planes_calls`,
    which stay attributes of the engine (the sinks bump them there).  Two hooks say what a frame is to the network; their defaults
    are HAT's: `_pad_multiple()`, the multiple a frame is reflect-padded to before the forward (the window size; 1: the network
    takes any size and refuses in its own words), and `_out_factor()`, the factor between a frame and its result (`scale`)."""

    def _pad_multiple(self) -> int:
        return self.ws

    def _out_factor(self) -> int:
        return self.scale

    def forward_ensemble(self, x: torch.Tensor, n: int = 8, *, one_stream: Optional[bool] = None) -> torch.Tensor:
        """The geometric self-ensemble ("+" mode; basicsr models/sr_model.py:132-178): the mean over the first n of the eight flips /
        transposes T_i of x of T_i^-1(forward(T_i x)), n in {1, 2, 4, 8} (ValueError otherwise).  Member i = v | h << 1 | t << 2
        (v: reverse W, h: reverse H, t: swap H and W, applied in that order).  Accumulated in fp32 in member order, acc += (1 / n) *
        T_i^-1(y_i); n = 1 is forward(x).  Shapes and refusals are forward's.  hat_dihedral_f32 makes every transformed input (into
        the workspace of the member's shape: the transposed members run a (B, W, H) workspace) and undoes, scales and adds every
        output in one pass; no torch op computes."""
        n = ops.ensemble_members(n)
        if not x.is_cuda:
            raise RuntimeError("HAT forward needs a device tensor: the HIP path is the only path")
        if x.device != self.dev:
            raise RuntimeError(f"input is on {x.device} but this engine's weights and workspace live on {self.dev}")
        with self._lock, torch.cuda.device(self.dev):
            if n == 1:
                return self._forward(x, one_stream=one_stream)
            self._check_input(x)
            # the result is the caller's, as forward's is: it is the accumulator (the byte paths, whose fp32 image never leaves
            # the engine, keep theirs in the workspace: _ens_acc)
            s = self._out_factor()
            acc = torch.empty(x.shape[0], x.shape[1], x.shape[2] * s, x.shape[3] * s, dtype=torch.float32, device=self.dev)
            return self._ensemble(x, n, acc, one_stream=one_stream)

    def _ws_buffer(self, ws, key, shape):
        """An fp32 buffer that lives in the per-shape workspace `ws`, allocated with its first use (as x_u8 is)."""
        t = ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = ws[key] = torch.zeros(shape, dtype=torch.float32, device=self.dev)
            ws["bytes"] += t.numel() * 4
        return t

    def _ens_acc(self, ws, B, Hp, Wp):
        """The byte paths' fp32 accumulator of the (B, Hp, Wp) workspace: the ensembled image before the crop and the conversion."""
        return self._ws_buffer(ws, "ens_acc", (B, 3, Hp * self._out_factor(), Wp * self._out_factor()))

    def _ensemble(self, x, n, acc, one_stream=None):
        """acc (B, C, sH, sW) fp32 = sum over i < n of (1 / n) * T_i^-1(forward(T_i x)), in member order; returns acc.  Called under
        the lock.  x must not be the buffer a member's input is written to (it is not: that is ens_x, this method's own)."""
        x = x.to(torch.float32).contiguous()
        B, C_, H, W = x.shape
        plan = getattr(self, "t16_fallbacks", 0)   # (HATEngine's FP16-range guard: a member that switches the engine to the fp32 stream ...)
        i = 0
        while i < n:
            if i == 0:
                xi = x
            else:
                Hi, Wi = (W, H) if i & 4 else (H, W)
                xi = self._ws_buffer(self._workspace(B, Hi, Wi), "ens_x", (B, C_, Hi, Wi))
                ops.dihedral(x, xi, op=i)
            y = self._forward(xi, one_stream=one_stream)
            if not y.is_contiguous():   # a corner of a larger buffer (ESCRealM behind its unshuffled stem): into the member's workspace
                Hi, Wi = xi.shape[2:]
                y = self._ws_buffer(self._workspace(B, Hi, Wi), "ens_y", tuple(y.shape)).copy_(y)
            if getattr(self, "t16_fallbacks", 0) != plan:   # (... starts the ensemble again: no member of it stays clipped)
                plan, again = self.t16_fallbacks, i > 0
                if again:
                    i = 0
                    continue
            ops.dihedral(y, acc, op=i, inverse=True, alpha=1.0 / n, accumulate=i > 0)
            i += 1
        return acc

    def _check_u8(self):
        if self.cfg["in_chans"] != 3:
            raise RuntimeError(f"8-bit frames are three-channel images: in_chans={self.cfg['in_chans']} has no uint8 path "
                               f"(use forward() and convert the planes yourself)")

    def _u8_out(self, out, shape):
        """The (B,h_out,w_out,3) uint8 result: the caller's `out` (rows may be pitched) or a fresh tensor."""
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.dev)
        if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != self.dev or out.stride(3) != 1 or out.stride(2) != 3:
            raise RuntimeError(f"out must be a {tuple(shape)} uint8 tensor on {self.dev} with interleaved pixels, got "
                               f"{tuple(out.shape)} {out.dtype} on {out.device}")
        return out

    def _to_sink(self, x, sink, ensemble, one_stream=None):
        """The forward of the planes x into `sink`, or their ensemble's (2 / 4 / 8: forward_ensemble's fp32 image in the workspace,
        then sink.from_planes).  Called under the lock; returns sink.out."""
        if ensemble > 1:
            B, _, Hp, Wp = x.shape
            sink.from_planes(self._ensemble(x, ensemble, self._ens_acc(self._workspace(B, Hp, Wp), B, Hp, Wp), one_stream=one_stream))
            return sink.out
        return self._forward(x, one_stream=one_stream, sink=sink)

    def _frame_forward(self, B, h, w, fill, make_sink, ensemble, what=None, of="frame"):
        """What the frame entry points share: (B, h, w) frames reflect-pad to the next window multiple (Hp, Wp) or are refused;
        fill(x) writes the padded fp32 planes x = ws["x_u8"], the one staging buffer of this shape's workspace; make_sink() checks
        the caller's `out` and returns the sink; then the forward (or its ensemble) into it."""
        m = self._pad_multiple()
        Hp, Wp = -(-h // m) * m, -(-w // m) * m
        if Hp - h >= h or Wp - w >= w:
            raise RuntimeError(f"{what or f'a {h}x{w} frame'} cannot be reflect-padded to {Hp}x{Wp} (window_size {self.ws}): the padding must be "
                               f"smaller than the {of}")
        sink = make_sink()
        with self._lock, torch.cuda.device(self.dev):
            x = self._ws_buffer(self._workspace(B, Hp, Wp), "x_u8", (B, 3, Hp, Wp))
            fill(x)
            return self._to_sink(x, sink, ensemble)

    def forward_to_u8(self, x: torch.Tensor, *, crop=None, bgr: bool = False, out=None, one_stream: Optional[bool] = None,
                      ensemble: int = 1) -> torch.Tensor:
        """forward(x) converted on the device as the reference's tensor2img converts it: (B,3,H,W) float in ->
        (B,h_out,w_out,3) uint8 out, crop = (h_out, w_out) the top-left pixels kept (default: all of (sH, sW)), bgr: bytes in
        B, G, R order, out: write into this tensor instead of a fresh one (then the call allocates nothing on the fused path).
        The fp32 image is not written where conv_last converts in its epilogue (u8_fused_calls counts those).
        ensemble 2 / 4 / 8: forward_ensemble's fp32 image (in the workspace), then hat_planes_to_u8 with the crop."""
        self._check_u8()
        ensemble = ops.ensemble_members(ensemble)
        if not x.is_cuda or x.device != self.dev:
            raise RuntimeError(f"HAT forward needs a tensor on {self.dev}: the HIP path is the only path")
        s = self._out_factor()
        ho, wo = (x.shape[2] * s, x.shape[3] * s) if crop is None else (int(crop[0]), int(crop[1]))
        if not (1 <= ho <= x.shape[2] * s and 1 <= wo <= x.shape[3] * s):
            raise RuntimeError(f"crop {(ho, wo)} does not lie inside the output {(x.shape[2] * s, x.shape[3] * s)}")
        with self._lock, torch.cuda.device(self.dev):
            if ensemble > 1:
                self._check_input(x)
            return self._to_sink(x, _U8Sink(self, self._u8_out(out, (x.shape[0], ho, wo, 3)), bgr), ensemble, one_stream)

    def forward_u8(self, frame: torch.Tensor, *, bgr: bool = False, out=None, ensemble: int = 1) -> torch.Tensor:
        """(B,h,w,3) uint8 device frames of any size the reflection allows -> (B,s*h,s*w,3) uint8: float(v) / 255, the
        reflect-pad to the next window multiple (hat_u8_to_planes, into this shape's workspace), the forward, the crop and
        tensor2img's conversion (in conv_last's epilogue or hat_planes_to_u8).  bgr: the bytes are B, G, R on both sides;
        out: the caller's (B,s*h,s*w,3) uint8 result tensor (default: a fresh one).  ensemble 2 / 4 / 8: the padded planes go
        through forward_ensemble (pad first, ensemble the padded image, crop last), then hat_planes_to_u8."""
        self._check_u8()
        ensemble = ops.ensemble_members(ensemble)
        if frame.dim() != 4 or frame.shape[3] != 3 or frame.dtype != torch.uint8:
            raise RuntimeError(f"expected (B,h,w,3) uint8 frames, got {tuple(frame.shape)} {frame.dtype}")
        if not frame.is_cuda or frame.device != self.dev:
            raise RuntimeError(f"HAT forward needs a tensor on {self.dev}: the HIP path is the only path")
        B, h, w, _ = frame.shape
        if frame.stride(3) != 1 or frame.stride(2) != 3:
            frame = frame.contiguous()
        return self._frame_forward(B, h, w, lambda x: ops.u8_to_planes(frame, x, bgr=bgr),
                                   lambda: _U8Sink(self, self._u8_out(out, (B, h * self._out_factor(), w * self._out_factor(), 3)), bgr), ensemble)

    def forward_gt_u8(self, gt: torch.Tensor, *, bgr: bool = False, out=None, ensemble: int = 1) -> torch.Tensor:
        """(B,H,W,3) uint8 device GROUND-TRUTH frames -> the (B, H - H % s, W - W % s, 3) uint8 super-resolution of their own
        bicubic low-resolution image, as the reference's GT-only dataset makes it (hat/data/imagenet_paired_dataset.py:49-59):
        mod-crop to multiples of the upscale s (a view, no copy), resize.imresize_u8 at 1 / s (ops.imresize: float,
        unrounded, with its overshoot) written reflect-padded into this shape's workspace, the forward, the crop and
        tensor2img's conversion as in forward_u8.  bgr, out, ensemble: as in forward_u8."""
        self._check_u8()
        ensemble = ops.ensemble_members(ensemble)
        if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or gt.dim() != 4 or gt.shape[3] != 3:
            raise RuntimeError(f"expected (B,H,W,3) uint8 ground-truth frames, got {tuple(getattr(gt, 'shape', ()))} {getattr(gt, 'dtype', type(gt))}")
        if not gt.is_cuda or gt.device != self.dev:
            raise RuntimeError(f"HAT forward needs a tensor on {self.dev}: the HIP path is the only path")
        s = self._out_factor()
        if s not in (2, 3, 4):
            raise RuntimeError(f"forward_gt_u8 makes the low-resolution image at 1/2, 1/3 or 1/4: upscale {s} has no such path")
        B, H, W, _ = gt.shape
        if gt.stride(3) != 1 or gt.stride(2) != 3:
            gt = gt.contiguous()
        gt = gt[:, :H - H % s, :W - W % s]
        h, w = gt.shape[1] // s, gt.shape[2] // s
        return self._frame_forward(B, h, w, lambda x: ops.imresize(gt, 1.0 / s, dst=x, pad_to=tuple(x.shape[2:]), bgr=bgr),
                                   lambda: _U8Sink(self, self._u8_out(out, (B, h * s, w * s, 3)), bgr), ensemble,
                                   what=f"the {h}x{w} low-resolution image of a {H}x{W} frame", of="image")

    def forward_yuv420(self, frame: torch.Tensor, *, fmt: str = "nv12", to_rgb, from_rgb, out=None, depth: int = 8, out_depth=None,
                       msb=None, ensemble: int = 1, siting: str = "center", out_siting=None) -> torch.Tensor:
        """forward_yuv for the three 4:2:0 layouts of yuv.FORMATS, the same one on both sides: (B,3h/2,w) device frames in the
        layout `fmt`, h and w even -> (B,3sh/2,sw) in the same layout; msb: the alignment of deep words on both sides (default: by
        the layout).  It refuses what is no 4:2:0 frame in its own words; everything else is forward_yuv's."""
        self._check_u8()
        ensemble = ops.ensemble_members(ensemble)
        from . import yuv as _yuv
        _yuv.check_fmt(fmt)
        out_depth = depth if out_depth is None else out_depth
        _yuv.container(depth, fmt, msb), _yuv.container(out_depth, fmt, msb)   # (checks the depths)
        in_dt = torch.uint8 if depth == 8 else torch.uint16
        if not isinstance(frame, torch.Tensor) or frame.dtype not in (torch.uint8, torch.uint16):
            raise TypeError(f"expected (B,3h/2,w) uint8 frames, got {getattr(frame, 'dtype', type(frame))}")
        if frame.dtype != in_dt:
            raise TypeError(f"{depth}-bit frames are {in_dt} tensors (uint8 holds 8-bit samples, uint16 deeper ones), got {frame.dtype}")
        if frame.dim() != 3:
            raise RuntimeError(f"expected (B,3h/2,w) uint8 frames, got {tuple(frame.shape)}")
        if not frame.is_cuda or frame.device != self.dev:
            raise RuntimeError(f"HAT forward needs a tensor on {self.dev}: the HIP path is the only path")
        _yuv.frame_size(frame.shape)
        return self.forward_yuv(frame, fmt=fmt, out_fmt=fmt, to_rgb=to_rgb, from_rgb=from_rgb, out=out, depth=depth, out_depth=out_depth,
                                msb=msb, out_msb=msb, ensemble=ensemble, siting=siting, out_siting=out_siting)

    def forward_yuv(self, frame: torch.Tensor, *, fmt: str, out_fmt=None, to_rgb, from_rgb, out=None, depth: int = 8, out_depth=None,
                    msb=None, out_msb=None, ensemble: int = 1, siting: str = "center", out_siting=None, width=None) -> torch.Tensor:
        """(B,rows,w) device frames in the layout `fmt` of yuv.LAYOUTS or yuv.PACKED_FORMATS, any size the layout and the reflection
        allow -> the frames of the s-times larger image in the layout `out_fmt` (default: fmt), any subsampling, grey or packed
        4:2:2 to any other: hat_yuv_to_planes (hat_packed422_to_planes) into this shape's workspace, the forward, the crop and the
        conversion back (in conv_last's epilogue, hat_conv3x3_to_yuv, or hat_planes_to_yuv / hat_planes_to_packed422).  to_rgb /
        from_rgb: yuv.csc's matrices (of `depth` / `out_depth`).  out: the caller's result tensor.  depth / out_depth 10, 12, 16:
        uint16 frames on that side (yuv.py, "Deep samples"; out_depth defaults to depth; a v210 side has depth 10 and uint8 frames);
        msb / out_msb: MSB-aligned words on that side (default: by the layout).  ensemble 2 / 4 / 8: the padded RGB planes go through
        forward_ensemble, then the from-planes kernel with the crop.  siting / out_siting (yuv.SITINGS; out_siting defaults to
        siting): the chroma siting of each side; a co-sited or packed output ends in hat_conv3x3_to_planes and the from-planes kernel
        (yuv_planes_calls counts it), never in conv_last's epilogue.  width: the source's width in pixels, required where fmt is
        'v210' (ValueError without it) and checked for every other layout."""
        self._check_u8()
        ensemble = ops.ensemble_members(ensemble)
        out_siting = siting if out_siting is None else out_siting
        src = ops.FrameSide(fmt, depth=depth, msb=msb, siting=siting)
        dst = ops.FrameSide(fmt if out_fmt is None else out_fmt, depth=depth if out_depth is None else out_depth, msb=out_msb, siting=out_siting)
        if not isinstance(frame, torch.Tensor) or frame.dtype not in (torch.uint8, torch.uint16):
            raise TypeError(f"expected (B,rows,w) uint8 frames, got {getattr(frame, 'dtype', type(frame))}")
        if frame.dtype != src.dtype:
            raise TypeError(f"{src.depth}-bit {fmt} frames are {src.dtype} tensors (uint8 holds 8-bit samples and v210 rows, uint16 deeper ones), "
                            f"got {frame.dtype}")
        if frame.dim() != 3:
            raise RuntimeError(f"expected (B,rows,w) {fmt} frames, got {tuple(frame.shape)}")
        if not frame.is_cuda or frame.device != self.dev:
            raise RuntimeError(f"HAT forward needs a tensor on {self.dev}: the HIP path is the only path")
        h, w = src.size(frame.shape, width)
        B, s = frame.shape[0], self._out_factor()
        return self._frame_forward(B, h, w, lambda x: src.to_planes(frame, x, to_rgb, width=w),
                                   lambda: yuv_sink(self, dst.out(out, (B,) + dst.shape(s * h, s * w), self.dev), dst, from_rgb, s * w), ensemble)
