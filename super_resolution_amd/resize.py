"""MATLAB-style bicubic imresize: the DEFINITION, on the host, of what csrc/hat_resize.hip computes.

This is the resize every published SR number starts from: the reference makes its low-resolution input with
`imresize(img_gt, 1 / scale)` (basicsr/utils/matlab_functions.py:16-178, MATLAB's antialiased bicubic; used by
hat/data/imagenet_paired_dataset.py:59).  It is separable: one table of weights and source indices per axis, the H pass
first, then the W pass (matlab_functions.py:142-169).

Tables.  weights_indices(in_len, out_len, scale, antialiasing) -> (w, src): float32 (out_len, P) weights and int32
(out_len, P) source indices.  The weights are built with torch fp32 CPU ops in the reference's order of operations
(matlab_functions.py:27-82): linspace(1, out_len), u = x / scale + 0.5 (1 - 1 / scale), left = floor(u - kw / 2) with
kw = 4 (4 / scale when shrinking with antialiasing), P = ceil(kw) + 2 columns, the cubic with its two branches (scaled by
`scale` when antialiasing), each row divided by its sum, and an all-zero first or last column dropped (the reference's
narrow() then drops BOTH outer columns when the first is zero, :71-73; so does this).  They equal the reference's bit for
bit; the kernels take them from the host for that reason: the device's linspace, division and floor need not round alike.
The reference then copies sym_len_s = 1 - min(index) mirrored rows in front of the image and sym_len_e = max(index) -
in_len behind it (:79-81, :129-140) and reads the augmented image.  Here the copy is folded into the index: with
s = (1-based index) - 1, src = -s - 1 for s < 0, 2 in_len - 1 - s for s >= in_len, s otherwise.  The reference mirrors the
INTERMEDIATE of the H pass before the W pass (:151-162); the H pass works column by column, so that is the same rule
applied to the source columns.  sym_len_s > in_len or sym_len_e > in_len is a ValueError: the mirror would need more
pixels than the image has (the reference's slicing silently breaks there).

Pixels.  imresize: out1[c,i,x] = sum_k w_h[i,k] * img[c, src_h[i,k], x], k ascending from a zero accumulator, and
out[c,i,j] = sum_k w_w[j,k] * out1[c,i,src_w[j,k]] likewise.  Every product and every sum is rounded to fp32 on its own
(numpy float32 arithmetic does exactly that; the kernels compile with floating-point contraction off), so the device
results EQUAL these bit for bit and the tests compare with torch.equal.  No clamp, no rounding: a bicubic overshoots, and
the reference hands the overshoot to the network.  Against the reference itself only a bound can hold: it sums with
Tensor.mv, whose order is unspecified.  With S = max_i sum_k |w[i,k]| per axis the bound is
(P_h S_h + P_w S_w S_h) 2^-24 max|img| (error_bound below).

out_len = ceil(in_len * scale) (matlab_functions.py:118).

Command line: python -m super_resolution_amd.resize -i DIR -o DIR --scale 0.25 [--no-antialiasing] [--mod-crop N]
writes the 8-bit LR PNG set of a folder (the usual "generate LR" step), uint8 to uint8 on the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch

_F = np.float32


def _cubic(x: torch.Tensor) -> torch.Tensor:      # matlab_functions.py:6-13
    a = torch.abs(x)
    a2 = a ** 2
    a3 = a ** 3
    inner = (a <= 1).type_as(a)
    outer = ((a > 1) * (a <= 2)).type_as(a)
    return (1.5 * a3 - 2.5 * a2 + 1) * inner + (-0.5 * a3 + 2.5 * a2 - 4 * a + 2) * outer


def out_length(in_len: int, scale: float) -> int:
    return int(math.ceil(in_len * scale))


def tables(in_len: int, out_len: int, scale: float, antialiasing: bool = True):
    """(w float32 (out_len,P), s int64 (out_len,P) UNMIRRORED 0-based source positions, sym_len_s, sym_len_e)."""
    in_len, out_len, scale = int(in_len), int(out_len), float(scale)
    if in_len < 1 or out_len < 1 or not scale > 0:
        raise ValueError(f"imresize needs positive lengths and a positive scale, got {in_len} -> {out_len} at {scale}")
    shrink = scale < 1 and antialiasing
    kw = 4 / scale if shrink else 4
    x = torch.linspace(1, out_len, out_len)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kw / 2)
    p = math.ceil(kw) + 2
    idx = left.view(out_len, 1).expand(out_len, p) + torch.linspace(0, p - 1, p).view(1, p).expand(out_len, p)
    dist = u.view(out_len, 1).expand(out_len, p) - idx
    w = scale * _cubic(dist * scale) if shrink else _cubic(dist)
    w = w / torch.sum(w, 1).view(out_len, 1).expand(out_len, p)
    zeros = torch.sum((w == 0), 0)
    if int(zeros[0]) != 0:
        idx, w = idx.narrow(1, 1, p - 2), w.narrow(1, 1, p - 2)
    if int(zeros[-1]) != 0:
        idx, w = idx.narrow(1, 0, p - 2), w.narrow(1, 0, p - 2)
    sym_s = int(-idx.min() + 1)
    sym_e = int(idx.max() - in_len)
    if sym_s > in_len or sym_e > in_len:
        raise ValueError(f"imresize of length {in_len} at scale {scale} would mirror {max(sym_s, sym_e)} pixels: the image is too small")
    return w.contiguous().numpy().astype(_F), idx.contiguous().numpy().astype(np.int64) - 1, sym_s, sym_e


def mirror(s: np.ndarray, in_len: int) -> np.ndarray:
    """The symmetric copy as an index rule: positions before the image read -s - 1, positions behind it 2 in_len - 1 - s."""
    return np.where(s < 0, -s - 1, np.where(s >= in_len, 2 * in_len - 1 - s, s))


def weights_indices(in_len: int, out_len: int, scale: float, antialiasing: bool = True):
    """(w, src): float32 (out_len, P) weights, int32 (out_len, P) source indices with the symmetric copy folded in."""
    w, s, _, _ = tables(in_len, out_len, scale, antialiasing)
    return w, mirror(s, int(in_len)).astype(np.int32)


def smallest_length(scale: float, antialiasing: bool = True, limit: int = 4096) -> int:
    """The smallest in_len that weights_indices accepts at this scale."""
    for n in range(1, limit):
        try:
            tables(n, out_length(n, scale), scale, antialiasing)
            return n
        except ValueError:
            continue
    raise ValueError(f"no length below {limit} can be resized at scale {scale}")


def _pass(img: np.ndarray, w: np.ndarray, src: np.ndarray, axis: int) -> np.ndarray:
    """One separable pass along `axis` of a (c, h, w) array: k ascending from zero, products and sums rounded one by one."""
    shape = list(img.shape)
    shape[axis] = w.shape[0]
    acc = np.zeros(shape, dtype=_F)
    for k in range(w.shape[1]):
        wk = w[:, k].reshape((-1, 1) if axis == 1 else (1, -1))
        acc = acc + wk * np.take(img, src[:, k], axis=axis)
    return acc


def imresize(img: np.ndarray, scale: float, antialiasing: bool = True, *, layout: str = "chw") -> np.ndarray:
    """float32 (c,h,w) (layout='chw') or (h,w,c) ('hwc') of any range -> the resized image in the same layout."""
    img = np.asarray(img)
    if img.dtype != _F or img.ndim != 3 or layout not in ("chw", "hwc"):
        raise ValueError(f"imresize takes a float32 (c,h,w) or (h,w,c) array, got {img.shape} {img.dtype} as {layout!r}")
    if layout == "hwc":
        return np.ascontiguousarray(imresize(np.ascontiguousarray(img.transpose(2, 0, 1)), scale, antialiasing).transpose(1, 2, 0))
    _, h, w = img.shape
    w_h, s_h = weights_indices(h, out_length(h, scale), scale, antialiasing)
    w_w, s_w = weights_indices(w, out_length(w, scale), scale, antialiasing)
    return _pass(_pass(img, w_h, s_h, 1), w_w, s_w, 2)


def u8_planes(frame: np.ndarray, *, bgr: bool = False) -> np.ndarray:
    """(h,w,3) uint8 -> (3,h,w) float32(v) / 255, the correctly rounded quotient (hat_u8_to_planes' table); bgr: the bytes
    are B, G, R and plane c is byte 2 - c."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"expected an (h,w,3) uint8 frame, got {frame.shape} {frame.dtype}")
    if bgr:
        frame = frame[:, :, ::-1]
    return np.ascontiguousarray((frame.astype(_F) / _F(255.0)).transpose(2, 0, 1))


def imresize_u8(frame: np.ndarray, scale: float, antialiasing: bool = True, *, bgr: bool = False) -> np.ndarray:
    """(h,w,3) uint8 -> float32 (3,oh,ow) planes: imresize of float32(v) / 255, unrounded and unclamped."""
    return imresize(u8_planes(frame, bgr=bgr), scale, antialiasing)


def to_u8(planes: np.ndarray, *, bgr: bool = False) -> np.ndarray:
    """float32 (3,h,w) planes -> (h,w,3) uint8: rint(clamp(v, 0, 1) * 255), half to even (hat_unit_to_u8's expression)."""
    v = np.minimum(np.maximum(np.asarray(planes, dtype=_F), _F(0.0)), _F(1.0)) * _F(255.0)
    out = np.rint(v).astype(np.uint8).transpose(1, 2, 0)
    return np.ascontiguousarray(out[:, :, ::-1] if bgr else out)


def error_bound(h: int, w: int, scale: float, antialiasing: bool = True, max_abs: float = 1.0) -> float:
    """The most two fp32 evaluations of imresize that sum in different orders can differ by, from the tables themselves:
    (P_h S_h + P_w S_w S_h) 2^-24 max|img| with S = max_i sum_k |w[i,k]|."""
    w_h, _ = weights_indices(h, out_length(h, scale), scale, antialiasing)
    w_w, _ = weights_indices(w, out_length(w, scale), scale, antialiasing)
    s_h = float(np.abs(w_h.astype(np.float64)).sum(1).max())
    s_w = float(np.abs(w_w.astype(np.float64)).sum(1).max())
    return (w_h.shape[1] * s_h + w_w.shape[1] * s_w * s_h) * 2.0 ** -24 * float(max_abs)


# ---- Pillow's 8-bit bicubic `Image.resize` (libImaging/Resample.c): the DEFINITION of what csrc/hat_pil_resize.hip computes.
# A sibling of the MATLAB tables above, not a mode of them: the scale is per axis (in / out), nothing is mirrored (the window is
# cut at the image's edge and renormalised), the coefficients are 22-bit fixed point and the image between the two passes is
# uint8.  The ESC-LTE benchmark's LR images are made with it (esc_arb/datasets/wrappers.py:149-152).
PIL_PRECISION_BITS = 32 - 8 - 2   # Resample.c: PRECISION_BITS


def _pil_bicubic(x: float) -> float:   # Resample.c: bicubic_filter, a = -0.5
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_tables(in_len: int, out_len: int):
    """One axis of Pillow's 8-bit bicubic resize: (coef int32 (out_len, K), bounds int32 (out_len, 2) = (first tap, tap count)),
    K = 2 ceil(2 max(in / out, 1)) + 1; output i is clip8((2^21 + sum_k coef[i,k] * pixel[first + k]) >> 22) over its tap count.
    Float64 arithmetic in Pillow's order of operations (precompute_coeffs, normalize_coeffs_8bpc)."""
    in_len, out_len = int(in_len), int(out_len)
    if in_len < 1 or out_len < 1:
        raise ValueError(f"a resize needs positive lengths, got {in_len} -> {out_len}")
    scale = in_len / out_len
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((out_len, ksize), dtype=np.int32)
    bounds = np.zeros((out_len, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_len):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_len) - xmin
        k = [_pil_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        coef[xx, :xmax] = [int(-0.5 + v * (1 << PIL_PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_PRECISION_BITS)) for v in k]
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def _pil_pass(img: np.ndarray, coef: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of a (n, ...) uint8 array -> (out_len, ...) uint8, in integers."""
    out = np.empty((coef.shape[0],) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    tail = (1,) * (img.ndim - 1)
    for i in range(coef.shape[0]):
        first, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (coef[i, :n].astype(np.int64).reshape((n,) + tail) * src[first:first + n]).sum(0) + (1 << (PIL_PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PIL_PRECISION_BITS, 0, 255)
    return out


def pil_bicubic_u8(img_u8: np.ndarray, size) -> np.ndarray:
    """(h,w,3) uint8 -> (size[0], size[1], 3) uint8, equal bit for bit to PIL.Image.resize((size[1], size[0]), BICUBIC) of the RGB
    image: the horizontal pass into a uint8 image first, then the vertical pass."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"expected an (h,w,3) uint8 frame, got {img.shape} {img.dtype}")
    oh, ow = int(size[0]), int(size[1])
    mid = _pil_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), *pil_tables(img.shape[1], ow)).transpose(1, 0, 2)
    return np.ascontiguousarray(_pil_pass(np.ascontiguousarray(mid), *pil_tables(img.shape[0], oh)))


def mod_crop(h: int, w: int, n: int):
    return h - h % n, w - w % n


def main(argv=None):
    import argparse
    import os

    from . import ops
    from .data import _scan, write_image
    ap = argparse.ArgumentParser(description="Write the 8-bit bicubic LR set of a folder of images (MATLAB imresize, on the device).")
    ap.add_argument("-i", "--input", required=True, help="folder of ground-truth images")
    ap.add_argument("-o", "--output", required=True, help="folder for the resized PNGs (same basenames)")
    ap.add_argument("--scale", type=float, required=True, help="resize factor, e.g. 0.25")
    ap.add_argument("--no-antialiasing", action="store_true")
    ap.add_argument("--mod-crop", type=int, default=0, metavar="N", help="crop height and width to multiples of N first")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from PIL import Image
    dev = torch.device(args.device)
    n = 0
    for path in _scan(args.input):
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if args.mod_crop > 0:
            hh, ww = mod_crop(a.shape[0], a.shape[1], args.mod_crop)
            a = a[:hh, :ww]
        frame = torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(0).to(dev)
        with torch.cuda.device(dev):
            out = ops.imresize(frame, args.scale, antialiasing=not args.no_antialiasing, to="u8")
        write_image(out[0].cpu().numpy(), os.path.join(args.output, os.path.splitext(os.path.basename(path))[0] + ".png"))
        n += 1
    print(f"{n} images -> {args.output}")
    return n


if __name__ == "__main__":
    main()
