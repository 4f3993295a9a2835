"""Frame sequences: 8-bit host frames in, 8-bit host frames out, with the copies hidden behind the compute.

    for out in frames.upscale_frames(net, reader, bgr=True):   # reader yields (h,w,3) uint8 arrays of one size
        writer.write(out)

Two pinned input and two pinned output buffers, two device buffers on each side, and ONE extra stream for the copies of
both directions: while frame n computes on the current stream, frame n+1 uploads and frame n-1 downloads on the copy
stream; HIP events order the two streams.  No threads, no second process.  With the engine's own side stream the process
uses three streams, within the four hardware queues a process gets by default.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch


PIXFMTS = ("rgb24", "nv12", "nv21", "i420", "i422", "nv16", "i444", "nv24", "gray", "uyvy", "yuy2", "y210", "v210")


def _raw(t):
    """A uint16 tensor as int16 (the same words): torch's copy kernels are complete for the signed type."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def sync_guard(net):
    """The context in which `net`'s forwards run the FP16-range guard of the residual stream in "sync" mode (HATEngine.guard_mode;
    DESIGN 4.0c): for callers that bring every frame to the host anyway, so a frame whose stream left the FP16 range is run
    again on the fp32 stream before it is delivered.  Nothing for an engine without the guard, or with the guard "off"."""
    eng = net.engine()
    if getattr(eng, "_guard", None) is None or eng.t16_guard == "off":
        return contextlib.nullcontext()
    return eng.guard_mode("sync")


def fixed_scale_family(net) -> bool:
    """`net` is a fixed-scale network of the ESC family (ESC, ESCReal, ESCRealM, ESCFP): its frame paths are `upscale_*` and it is
    not marked `arbitrary_scale` (ESCLTE, whose `upscale_*` calls take size= / scale=)."""
    return hasattr(net, "upscale_u8") and not getattr(net, "arbitrary_scale", False)


def entry_points(net, arb: bool = False):
    """The names of (byte call, YCbCr call, 4:2:0 call or None) of `net` for upscale_frames: HAT's forward_u8 / forward_yuv / forward_yuv420; for a
    fixed-scale network of the ESC family (it has `upscale_u8` and is not marked `arbitrary_scale`) its upscale_u8 / upscale_yuv, the
    4:2:0 layouts through upscale_yuv too; with arb (size= / scale=) the network must be marked `arbitrary_scale` (ESCLTE)."""
    marked = bool(getattr(net, "arbitrary_scale", False))
    if arb and not marked:
        raise RuntimeError(f"upscale_frames: size= / scale= need an arbitrary-scale network with upscale_u8 / upscale_yuv (ESCLTE); "
                           f"{type(net).__name__} has a fixed scale")
    if arb or fixed_scale_family(net):
        return "upscale_u8", "upscale_yuv", None
    return "forward_u8", "forward_yuv", "forward_yuv420"


def upscale_frames(net, frames, *, bgr: bool = False, pixfmt: str = "rgb24", matrix: str = "bt601", full_range: bool = False, depth: int = 8,
                   out_depth=None, msb=None, ensemble: int = 1, out_pixfmt=None, out_msb=None, siting: str = "center", out_siting=None,
                   size=None, scale=None, width=None):
    """Generator: for every (h,w,3) uint8 array of `frames` (all of one size) yield the (s*h,s*w,3) uint8 array that
    `net.forward_u8` computes for it, in order.  `net`: a HAT / HATX module on a GPU, in eval mode.  The yielded array is
    the caller's own (copied out of the pinned buffer).  An empty sequence yields nothing.
    pixfmt 'nv12' / 'nv21' / 'i420': the frames are (3h/2, w) uint8 arrays in that 4:2:0 layout (yuv.py), the yielded arrays
    (3sh/2, sw) ones, computed by `net.forward_yuv420` with `matrix` and `full_range` (bgr does not apply).  Same slots,
    same copy stream, same events: only the buffer shapes and the forward differ.  depth / out_depth / msb (4:2:0 only): as
    HAT.forward_yuv420 takes them; a deep side's frames are uint16 arrays, and so are its pinned and device buffers.
    pixfmt 'i422' / 'nv16' / 'i444' / 'nv24' / 'gray', or out_pixfmt (any layout of yuv.LAYOUTS; default: pixfmt) different from
    pixfmt: the frames are arrays of yuv.frame_shape_fmt in that layout and every frame goes through `net.forward_yuv` (any
    subsampling in, any out; out_msb: the output words' alignment), in the same two-slot pipeline.
    pixfmt / out_pixfmt 'uyvy' / 'yuy2' / 'y210' / 'v210' (yuv.PACKED_FORMATS; depth 8, 8, 10 / 12 / 16, 10 on that side): packed 4:2:2
    frames, arrays of yuv.packed_shape, through `net.forward_yuv` in the same pipeline; width=: the frames' width in pixels, required
    for 'v210' frames (the array does not give it) and checked for every other YCbCr pixfmt.
    ensemble 2 / 4 / 8: every frame through the geometric self-ensemble (HAT.forward_ensemble) of that many members.
    siting / out_siting (YCbCr pixel formats; yuv.SITINGS): the chroma siting of the frames and of the yielded frames (default:
    the input's), as HAT.forward_yuv takes them; 'center' is the sequence as it always was.
    size=(h, w) or scale= (one of them): `net` is an arbitrary-scale network (ESCLTE) and every frame goes through `net.upscale_u8`
    (rgb24) or `net.upscale_yuv` (every YCbCr pixfmt) to that size, in the same two-slot pipeline; the yielded arrays have the
    resolved size's shape.  ensemble is then refused, and so is a network that is not marked `arbitrary_scale`.
    A fixed-scale network of the ESC family (ESC, ESCReal, ESCRealM, ESCFP: it has `upscale_u8` and is not `arbitrary_scale`) goes,
    without size= / scale=, through `net.upscale_u8` (rgb24) or `net.upscale_yuv` (every YCbCr pixfmt, the 4:2:0 ones included) with
    every keyword above, ensemble too, in the same two-slot pipeline; the yielded frames are `net.upscale` times the input's."""
    from .ops import ensemble_members
    ensemble = ensemble_members(ensemble)
    if pixfmt not in PIXFMTS:
        raise RuntimeError(f"unknown pixfmt {pixfmt!r}: one of {PIXFMTS}")
    if out_pixfmt is not None and (out_pixfmt not in PIXFMTS or (out_pixfmt == "rgb24") != (pixfmt == "rgb24")):
        raise RuntimeError(f"out_pixfmt {out_pixfmt!r}: one of {PIXFMTS[1:]} for a YCbCr pixfmt (rgb24 frames stay rgb24)")
    if out_msb is not None and pixfmt == "rgb24":
        raise RuntimeError("out_msb belongs to the YCbCr pixel formats")
    from . import yuv as _yuv
    out_siting = _yuv.check_siting(siting) if out_siting is None else _yuv.check_siting(out_siting)
    skw = {} if (siting, out_siting) == ("center", "center") else {"siting": siting, "out_siting": out_siting}
    if skw and pixfmt == "rgb24":
        raise RuntimeError("siting and out_siting belong to the YCbCr pixel formats")
    if width is not None and pixfmt == "rgb24":
        raise RuntimeError("width belongs to the YCbCr pixel formats (a v210 frame does not give its own)")
    arb = size is not None or scale is not None
    if arb:
        entry_points(net, arb=True)
        if (size is None) == (scale is None):
            raise ValueError("upscale_frames takes exactly one of size=(h, w) and scale=, or neither")
        if ensemble != 1:
            raise RuntimeError("upscale_frames: the self-ensemble is not built for size= / scale= (ESCLTE's frame paths)")
    name_u8, name_yuv, name_yuv420 = entry_points(net, arb)
    family = not arb and name_yuv420 is None   # a fixed-scale network of the ESC family
    general = pixfmt != "rgb24" and (arb or family or pixfmt not in PIXFMTS[1:4] or out_pixfmt not in (None, pixfmt) or out_msb is not None)
    yuv420 = pixfmt != "rgb24" and not general
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("upscale_frames needs the network on a GPU: the MI355X HIP path is the only path")
    it = iter(frames)
    first = next(it, None)
    if first is None:
        return
    first = np.ascontiguousarray(first)
    s = None if arb else net.upscale

    def out_hw(h, w):
        """The output size of an (h, w) frame: the network's scale, or the resolved size= / scale= (ESCLTE.upscale's rule)."""
        if not arb:
            return s * h, s * w
        return (int(h * scale), int(w * scale)) if size is None else (int(size[0]), int(size[1]))

    in_np, in_dt, out_dt = np.uint8, torch.uint8, torch.uint8
    if general:
        from . import yuv as _yuv
        if family and pixfmt in PIXFMTS[1:4] and out_pixfmt in (None, pixfmt) and out_msb is None:
            out_msb = msb   # (what forward_yuv420 makes of msb: the alignment of both sides)
        out_pixfmt = pixfmt if out_pixfmt is None else out_pixfmt
        out_depth = depth if out_depth is None else out_depth
        from .ops import FrameSide
        a, b = FrameSide(pixfmt, depth=depth, msb=msb, siting=siting), FrameSide(out_pixfmt, depth=out_depth, msb=out_msb, siting=out_siting)
        in_dt, out_dt = a.dtype, b.dtype
        in_np = np.uint8 if in_dt is torch.uint8 else np.uint16
        if first.ndim != 2 or first.dtype != in_np:
            raise RuntimeError(f"expected (rows,w) {np.dtype(in_np).name} {pixfmt} frames, got {first.shape} {first.dtype}")
        h, w = a.size(first.shape, width)
        in_shape, shape_text = first.shape, str(tuple(first.shape)).replace(" ", "")
        if arb:
            oh, ow = out_hw(h, w)
            if oh < 1 or ow < 1 or b.size_refusal(oh, ow):
                raise ValueError(f"upscale_frames: an output of {oh}x{ow} is no {out_pixfmt} frame")
        out_shape = b.shape(*out_hw(h, w))
        if width is not None:
            skw = dict(skw, width=w)
        if arb:
            forward = lambda src, dst: getattr(net, name_yuv)(src, size=out_hw(h, w), fmt=pixfmt, out_fmt=out_pixfmt, matrix=matrix, full_range=full_range,
                                                       out=dst, depth=depth, out_depth=out_depth, msb=msb, out_msb=out_msb, siting=siting,
                                                       out_siting=out_siting, **({} if width is None else {"width": w}))
        else:
            forward = lambda src, dst: getattr(net, name_yuv)(src, fmt=pixfmt, out_fmt=out_pixfmt, matrix=matrix, full_range=full_range, out=dst,
                                                       depth=depth, out_depth=out_depth, msb=msb, out_msb=out_msb, ensemble=ensemble, **skw)
    elif yuv420:
        from . import yuv as _yuv
        out_depth = depth if out_depth is None else out_depth
        in_np = _yuv.container(depth, pixfmt, msb)[0]
        _yuv.container(out_depth, pixfmt, msb)
        in_dt, out_dt = (torch.uint8 if d == 8 else torch.uint16 for d in (depth, out_depth))
        if first.ndim != 2 or first.dtype != in_np:
            raise RuntimeError(f"expected (3h/2,w) {np.dtype(in_np).name} {pixfmt} frames, got {first.shape} {first.dtype}")
        h, w = _yuv.frame_size(first.shape)
        in_shape, out_shape, shape_text = first.shape, _yuv.frame_shape(s * h, s * w), f"({3 * h // 2},{w})"
        forward = lambda src, dst: getattr(net, name_yuv420)(src, fmt=pixfmt, matrix=matrix, full_range=full_range, out=dst, depth=depth,
                                                      out_depth=out_depth, msb=msb, ensemble=ensemble, **skw)
    else:
        if depth != 8 or out_depth not in (None, 8):
            raise RuntimeError("rgb24 frames are 8-bit: depth and out_depth belong to the 4:2:0 pixel formats")
        if first.ndim != 3 or first.shape[2] != 3 or first.dtype != np.uint8:
            raise RuntimeError(f"expected (h,w,3) uint8 frames, got {first.shape} {first.dtype}")
        h, w, _ = first.shape
        in_shape, out_shape, shape_text = (h, w, 3), out_hw(h, w) + (3,), f"({h},{w},3)"
        if arb and min(out_shape) < 1:
            raise ValueError(f"upscale_frames: an output of {out_shape[0]}x{out_shape[1]} is empty")
        if arb:
            forward = lambda src, dst: getattr(net, name_u8)(src, size=out_shape[:2], bgr=bgr, out=dst)
        else:
            forward = lambda src, dst: getattr(net, name_u8)(src, bgr=bgr, out=dst, ensemble=ensemble)
    # Nothing of the device state stays entered across a yield: the buffers and the copy stream are made once, and every step
    # enters the device and takes the stream that is current THEN, so a caller may switch device or stream between frames.
    with torch.cuda.device(dev):
        copy = torch.cuda.Stream(device=dev)
        hin = [torch.empty(in_shape, dtype=in_dt).pin_memory() for _ in range(2)]
        hout = [torch.empty(out_shape, dtype=out_dt).pin_memory() for _ in range(2)]
        din = [torch.empty((1,) + tuple(in_shape), dtype=in_dt, device=dev) for _ in range(2)]
        dout = [torch.empty((1,) + tuple(out_shape), dtype=out_dt, device=dev) for _ in range(2)]
        ev = lambda: torch.cuda.Event()
        up, done, down = [ev(), ev()], [ev(), ev()], [ev(), ev()]

    def upload(k, a):
        """frame -> pinned slot k -> device slot k, on the copy stream (after the compute that last read the slot)."""
        a = np.ascontiguousarray(a)
        if a.shape != tuple(in_shape) or a.dtype != in_np:
            raise RuntimeError(f"all frames of a sequence must be {shape_text} {np.dtype(in_np).name}, got {a.shape} {a.dtype}")
        up[k].synchronize()                    # the previous upload out of this pinned buffer has finished
        hin[k].numpy()[...] = a
        with torch.cuda.device(dev), torch.cuda.stream(copy):
            copy.wait_event(done[k])           # the forward that last read din[k] (frame n-2) has finished
            _raw(din[k]).copy_(_raw(hin[k]).unsqueeze(0), non_blocking=True)
            up[k].record(copy)

    def compute(k):
        """forward of slot k on the stream that is current now, then its download on the copy stream."""
        with torch.cuda.device(dev):
            comp = torch.cuda.current_stream(dev)
            comp.wait_event(up[k])
            comp.wait_event(down[k])           # dout[k] was last read by the download of frame n-2
            comp.wait_event(done[k ^ 1])       # the engine's workspace is shared: after frame n-1's forward, whatever stream it ran on
            with sync_guard(net):              # (the frame goes to the host: a clipped one is run again first)
                forward(din[k], dout[k])
            done[k].record(comp)               # din[k] is free again and dout[k] is complete
            with torch.cuda.stream(copy):
                copy.wait_event(done[k])
                _raw(hout[k]).copy_(_raw(dout[k])[0], non_blocking=True)
                down[k].record(copy)

    def collect(k):
        down[k].synchronize()
        return hout[k].numpy().copy()

    n = 0
    upload(0, first)
    nxt = next(it, None)
    while True:
        k = n & 1
        if nxt is not None:
            upload(k ^ 1, nxt)                 # frame n+1 goes up while frame n computes
        compute(k)
        if n >= 1:
            yield collect(k ^ 1)               # frame n-1 (its download ran beside frame n's launches)
        n += 1
        if nxt is None:
            break
        nxt = next(it, None)
    yield collect((n - 1) & 1)
