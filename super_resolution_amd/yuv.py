"""4:2:0 YCbCr frames <-> the network's fp32 RGB planes: the DEFINITION, in numpy on the host.

What a decoder hands over and an encoder takes back is 4:2:0 YCbCr (NV12, NV21, I420; 8, 10, 12 or 16 bits per sample), not
packed RGB.  The 8-bit case is described first; "Deep samples" below adds the sample width as one more parameter.  This
module says, operation by operation, what the device kernels (csrc/hat_yuv.hip, the yuv epilogue of csrc/hat_cabsq.hip)
compute: every product and every sum below is rounded to fp32 on its own (numpy float32 arithmetic does exactly that; the
kernels compile the shared conversion with floating-point contraction off), so the device results EQUAL these, bit for
bit, and the tests compare with array_equal.

Colour matrices.  csc(matrix, full_range) -> (to_rgb, from_rgb), two float32[12] arrays, row-major 3 x 4:
  to_rgb    rows R, G, B; columns Y, Cb, Cr, offset.  Byte units in, [0, 1] out.
  from_rgb  rows Y, Cb, Cr; columns R, G, B, offset.  [0, 1] in, byte units out.
'bt601' limited range (the default everywhere) is the reference's basicsr/utils/color_util.py: from_rgb holds
rgb2ycbcr's literals, to_rgb holds ycbcr2rgb's constants folded once in fp64.  The reference's inverse constants are
rounded to six digits: its offsets are not exactly -(16 m[c][0] + 128 m[c][1] + 128 m[c][2]) but 1e-6 .. 3e-6 off, more
than the 2e-6 this module is pinned to the reference with, so the offset is kept as a number of its own.  The chroma
samples are centred on 128 (every matrix has that centre); the luma offset is part of to_rgb's offset column, which is
added last, so the twelve floats are the whole conversion and the C entry points need no range flag.  'bt709' and
full_range=True are derived in fp64 from Kr / Kb (0.299 / 0.114 and 0.2126 / 0.0722), offset -16 / 219 or 0.

Input, per pixel (y, x) of the reflect-padded plane: the source pixel is (sy, sx) = (y < h ? y : 2 (h - 1) - y, likewise x)
— hat_u8_to_planes' rule — and its chroma sample is (sy >> 1, sx >> 1): every chroma sample covers its 2 x 2 luma block
(nearest).  With Cb' = float(Cb) - 128, Cr' = float(Cr) - 128 (exact in fp32)
    plane_c = min(max((((m[c][0] * float(Y) + m[c][1] * Cb') + m[c][2] * Cr') + m[c][3]), 0), 1).

Output, from the fp32 value v the float path would have stored: r, g, b = min(max(v, 0), 1);
    Y  = ((k[0][0] r + k[0][1] g) + k[0][2] b) + k[0][3]                       per pixel
    cb = (k[1][0] r + k[1][1] g) + k[1][2] b          (no offset), cr likewise  per pixel
    Cb = ((cb00 + cb01) + (cb10 + cb11)) * 0.25 + k[1][3]                       per 2 x 2 block: left + right, then top + bottom
and a byte is rint(min(max(., 0), 255)), round half to even.

Chroma siting: nearest up, box down is CENTRE-sited chroma (JPEG, MPEG-1, Y4M C420jpeg), and it is what every function computes
by default (siting="center").  "Chroma siting" below defines 'left' (MPEG-2, H.264, HEVC, AV1 4:2:0; all standard 4:2:2) and
'topleft' (BT.2020 / UHD HEVC).  Other chroma filters and tone mapping are out of scope; 4:2:2, 4:4:4 and grey are "Other
subsamplings" below.

Deep samples (HEVC Main10, AV1, VP9 profile 2).  A deep sample is a little-endian 16-bit word that holds an n-bit code, n =
depth in {10, 12, 16}; k = n - 8, maxcode = 2^n - 1, shift = 16 - n for an MSB-aligned container, else 0.
  MSB-aligned (P010 / P012 / P016: VCN, VA-API, D3D surfaces)    code = word >> shift (the low bits are ignored); word = code << shift
  LSB-aligned (yuv420p10le / p12le, Y4M C420p10 / C420p12)       code = min(word, maxcode) (saturates, never wraps); word = code
The default alignment is MSB for 'nv12' / 'nv21' and LSB for 'i420'; msb=True / False overrides it; at n = 16 both are the same.
Input: s = float32(code) * 2^-k (exact), Cb' = s_cb - 128, Cr' = s_cr - 128 (exact: at most 16 significant bits), then the
expression above on s.  Output: Y, the cb / cr terms and the box are computed exactly as above, in byte units, and then
    code = rint(min(max(v * 2^k, 0), maxcode)), half to even (the product is exact; k = 0 is the byte rule).
csc(matrix, full_range, depth): the matrices stay in BYTE units.  Limited range: an n-bit code is the 8-bit code times 2^k
(H.273), so the twelve floats do not depend on the depth (the reference's BT.601 literals included).  Full range: the code is
(2^n - 1) E' with chroma centre 2^(n-1) = 128 in s units, so (2^n - 1) / 2^k (255.75 at 10 bits) takes the place of 255.
'bt2020nc' is BT.2020 non-constant luminance (Kr 0.2627, Kb 0.0593; ffmpeg's name).  NO transfer function is applied anywhere:
the network sees the source's own transfer (gamma, PQ, HLG) and its output carries the same one.

Layouts of one frame, a (3 h / 2, w) uint8 array (uint16 for deep samples), h and w even:
  nv12  h rows of Y, then h / 2 rows of interleaved Cb, Cr
  nv21  h rows of Y, then h / 2 rows of interleaved Cr, Cb
  i420  h rows of Y, then the (h / 2, w / 2) Cb plane, then the Cr plane (each stored contiguously in h / 4 rows' worth of bytes)

Other subsamplings (the general functions: yuv_to_planes, planes_to_yuv, split_fmt, join_fmt, frame_shape_fmt, frame_size_fmt).
LAYOUTS maps every layout name to (sub_x, sub_y, kind): the chroma sample of source pixel (sy, sx) is (sy >> sub_y, sx >> sub_x).
  name              sub   one frame array                                                         deep default
  i420 nv12 nv21    1,1   (3h/2, w), as above                                                     as above
  i422              1,0   (2h, w): Y, then the (h, w/2) Cb plane, then Cr (Y4M C422, yuv422p[10le])  LSB
  nv16              1,0   (2h, w): Y, then h rows of interleaved Cb, Cr (P210 / P216)               MSB
  i444              0,0   (3h, w): the Y, Cb, Cr planes (Y4M C444, yuv444p[10le])                   LSB
  nv24              0,0   (3h, w): Y, then h rows of 2w interleaved samples Cb, Cr (P410 / P416)    MSB
  gray              none  (h, w): Y only (Y4M Cmono, gray[10le])                                    LSB
w is even where sub_x = 1 and h where sub_y = 1; every other size >= 1 is a frame (the reflection still needs pad < size).
Depths, container, decode / encode and csc apply unchanged.  In: as above with the layout's shifts; for 'gray' Cb' = Cr' = 0
exactly and the same expression follows.  Out: Y and the per-pixel cb, cr terms as above, then
    4:2:0  as above        4:2:2  C = (c0 + c1) * 0.5 + k[c][3], left + right        4:4:4  C = c + k[c][3]        gray  Y only
and the byte / code rule is unchanged.  For nv12 / nv21 / i420 the general functions return what the 4:2:0 pair returns.
4:1:1, 4:4:0, alpha planes and tone mapping are out of scope; packed 4:2:2 is "Packed 4:2:2" below.

Packed 4:2:2 (PACKED_FORMATS; packed_shape, packed_size, unpack422, pack422, packed_to_planes, planes_to_packed).  What capture
cards, cameras and 4:2:2 decoders deliver: one array per frame, luma and chroma interleaved, w even and >= 2, any h >= 1.
  uyvy   bytes Cb0 Y0 Cr0 Y1 per pixel pair, 8 bit; (h, 2w) uint8                                     (ffmpeg uyvy422)
  yuy2   bytes Y0 Cb0 Y1 Cr0, 8 bit; (h, 2w) uint8                                                   (ffmpeg yuyv422)
  y210   little-endian 16-bit words Y0 Cb0 Y1 Cr0, depth 10 / 12 / 16 (16: Y216), MSB-aligned by default; (h, 2w) uint16
  v210   10 bit only.  Six pixels in four little-endian 32-bit words, three codes each at bits 0-9, 10-19, 20-29:
         word 0 Cb0 Y0 Cr0, word 1 Y1 Cb1 Y2, word 2 Cr1 Y3 Cb2, word 3 Y4 Cr2 Y5.  A row is 128 ceil(w / 48) bytes; (h, that) uint8.
         Out: bits 30-31 of every word, every code of the last group past w and every byte from the last group to the end of the
         row are zero.  In: none of them is read for its value.  The shape does not give the width: width= is required.
The samples mean what the samples of a (sub_x, sub_y) = (1, 0) surface mean, so the two directions are DEFINED through 'i422':
  packed_to_planes(frame)  = yuv_to_planes(join_fmt(*unpack422(frame), "i422"), fmt="i422")
  planes_to_packed(planes) = pack422(*split_fmt(planes_to_yuv(planes, fmt="i422"), "i422"))
with the word alignment of the packed side (v210's codes are LSB-aligned words in between).  Sitings: 'center' (the default, as for
every other call) and 'left'; 'topleft' means 'left', as on every 4:2:2 surface.  Standard 4:2:2 video is LEFT-sited.

Chroma siting (siting= / out_siting=; SITINGS = 'center', 'left', 'topleft', C codes 0, 1, 2).  An axis is CO-SITED when it is
subsampled and the siting puts the chroma sample on the even luma sample: x where sub_x = 1 and the siting is 'left' or 'topleft',
y where sub_y = 1 and the siting is 'topleft'.  Every other axis keeps the centre rule above, so on 4:2:2 'topleft' is 'left', and
on 4:4:4 and grey every siting is 'center' (accepted, not refused).  siting="center" takes exactly the code path above.
In (chroma_up).  Source pixel (sy, sx), after the reflection; s[.][.] the chroma samples as float32(code) * 2^-k; (ch, cw) the
chroma plane's size:
    j = sx >> sub_x, j1 = min(j + (sx & 1), cw - 1) if x is co-sited, else j;      i, i1 likewise from sy, sub_y, ch
    c = ((s[i][j] + s[i][j1]) + (s[i1][j] + s[i1][j1])) * 0.25,     Cb' = c - 128 (Cr' likewise), then the per-pixel expression.
Every step is exact in fp32 (four integers of at most 16 bits, a power of two), so one formula is nearest, horizontal-linear
and bilinear: an even luma sample takes its chroma sample, an odd one the mean of its two neighbours; right and bottom edges clamp.
Out (chroma_down).  The per-pixel cb / cr terms c (no offset) of the cropped h_out x w_out pixels as above; every + rounds to fp32
on its own, 2 * and the power-of-two scales are exact.  Row tap of chroma column j in pixel row r:
    co-sited x   t_r[j] = (c[r][max(2j - 1, 0)] + c[r][2j + 1]) + 2 c[r][2j]          centred x   t_r[j] = c[r][2j] + c[r][2j + 1]
    4:2:2 'left' / 'topleft'   C = t_r[j] * 0.25 + k[c][3]
    4:2:0 'left'               C = (t_2i[j] + t_2i+1[j]) * 0.125 + k[c][3]
    4:2:0 'topleft'            C = ((t_max(2i-1,0)[j] + t_2i+1[j]) + 2 t_2i[j]) * 0.0625 + k[c][3]
(the [1 2 1] / 4 filter centred on the even sample).  Left and top edges replicate, no tap reads past the crop, and the byte /
code rule is unchanged.  Other filters (Lanczos, 3/4 - 1/4 vertical linear for centred axes), PAL-DV's alternating-line siting and
transfer functions are out of scope.
"""
from __future__ import annotations

import numpy as np

FORMATS = ("nv12", "nv21", "i420")
# name -> (sub_x, sub_y, kind); kind 'planar': Cb plane then Cr plane, 'semi': interleaved Cb, Cr, 'semi_vu': interleaved Cr, Cb,
# 'gray': no chroma (sub_x = sub_y = None)
LAYOUTS = {"nv12": (1, 1, "semi"), "nv21": (1, 1, "semi_vu"), "i420": (1, 1, "planar"), "i422": (1, 0, "planar"), "nv16": (1, 0, "semi"),
           "i444": (0, 0, "planar"), "nv24": (0, 0, "semi"), "gray": (None, None, "gray")}
ALL_FORMATS = tuple(LAYOUTS)
PACKED_FORMATS = ("uyvy", "yuy2", "y210", "v210")   # the index is the C code (include/hat_mi355x.h, HAT_PACKED_*)
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020nc": (0.2627, 0.0593)}   # Kr, Kb
DEPTHS = (8, 10, 12, 16)
SITINGS = ("center", "left", "topleft")   # the index is the C code (include/hat_mi355x.h, HAT_SITING_*)
_F = np.float32


def check_fmt(fmt: str) -> str:
    if fmt not in FORMATS:
        raise RuntimeError(f"unknown 4:2:0 format {fmt!r}: one of {FORMATS}")
    return fmt


def check_layout(fmt: str):
    """(sub_x, sub_y, kind) of any layout of LAYOUTS."""
    if fmt not in LAYOUTS:
        raise RuntimeError(f"unknown frame format {fmt!r}: one of {ALL_FORMATS}")
    return LAYOUTS[fmt]


def check_siting(siting) -> str:
    if not isinstance(siting, str) or siting not in SITINGS:
        raise RuntimeError(f"unknown chroma siting {siting!r}: one of SITINGS = {SITINGS}")
    return siting


def cosited(sub, siting):
    """(x, y): which axes of a layout with sub = (sub_x, sub_y) (None or (None, None): grey) are co-sited under `siting`."""
    siting = check_siting(siting)
    if sub is None or sub[0] is None:
        return False, False
    return bool(sub[0] == 1 and siting != "center"), bool(sub[1] == 1 and siting == "topleft")


def effective_siting(sub, siting) -> str:
    """The siting that a layout makes of `siting`: 'center' on 4:4:4 and grey, 'left' for 'topleft' on 4:2:2."""
    cx, cy = cosited(sub, siting)
    return "topleft" if cy else "left" if cx else "center"


def check_depth(depth) -> int:
    if isinstance(depth, bool) or depth not in DEPTHS:
        raise RuntimeError(f"unsupported sample depth {depth!r}: one of {DEPTHS}")
    return int(depth)


def container(depth: int, fmt: str = "nv12", msb=None):
    """(dtype, k, maxcode, shift) of a sample of `depth` bits in layout `fmt`: see "Deep samples" in the module docstring."""
    depth = check_depth(depth)
    kind = check_layout(fmt)[2]
    if depth == 8:
        return np.uint8, 0, 255, 0
    msb = kind.startswith("semi") if msb is None else bool(msb)
    return np.uint16, depth - 8, (1 << depth) - 1, (16 - depth) if msb else 0


def csc(matrix: str = "bt601", full_range: bool = False, depth: int = 8):
    """(to_rgb, from_rgb): float32[12] each, in byte units at every depth, see the module docstring."""
    if matrix not in MATRICES:
        raise RuntimeError(f"unknown colour matrix {matrix!r}: one of {tuple(MATRICES)}")
    depth = check_depth(depth)
    if matrix == "bt601" and not full_range:
        fr = np.array([[65.481, 128.553, 24.966, 16.0], [-37.797, -74.203, 112.0, 128.0], [112.0, -93.786, -18.214, 128.0]])
        # ycbcr2rgb: rgb255 = (ycc_bytes @ M) * 255 + off  ->  rgb = ycc_bytes @ M + off / 255
        M = np.array([[0.00456621, 0.00456621, 0.00456621], [0.0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0.0]])
        off = np.array([-222.921, 135.576, -276.836]) / 255.0
        to = np.empty((3, 4))
        to[:, :3] = M.T
        to[:, 3] = 128.0 * M[1] + 128.0 * M[2] + off                    # the chroma centre moves into Cb', Cr'
        return to.astype(_F).reshape(12), fr.astype(_F).reshape(12)
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    top = ((1 << depth) - 1) / float(1 << (depth - 8))          # the full-range code of E' = 1 in byte units: 255, 255.75, ...
    ys, cs, oy = (top, top, 0.0) if full_range else (219.0, 224.0, 16.0)
    fr = np.array([[ys * kr, ys * kg, ys * kb, oy],
                   [-cs * kr / (2 * (1 - kb)), -cs * kg / (2 * (1 - kb)), cs * 0.5, 128.0],
                   [cs * 0.5, -cs * kg / (2 * (1 - kr)), -cs * kb / (2 * (1 - kr)), 128.0]])
    to = np.array([[1 / ys, 0.0, 2 * (1 - kr) / cs, -oy / ys],
                   [1 / ys, -2 * kb * (1 - kb) / (kg * cs), -2 * kr * (1 - kr) / (kg * cs), -oy / ys],
                   [1 / ys, 2 * (1 - kb) / cs, 0.0, -oy / ys]])
    return to.astype(_F).reshape(12), fr.astype(_F).reshape(12)


# ------------------------------------------------------------------------------------------------ layouts
def frame_shape(h: int, w: int):
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise RuntimeError(f"4:2:0 frames need even sizes, got {h}x{w}")
    return (3 * h // 2, w)


def frame_size(shape):
    """(h, w) of a (3 h / 2, w) 4:2:0 frame array."""
    hh, w = int(shape[-2]), int(shape[-1])
    if hh < 3 or hh % 3 or w < 2 or w % 2:
        raise RuntimeError(f"a 4:2:0 frame is a (3h/2, w) array with even h and w, got {tuple(shape)}")
    return 2 * hh // 3, w


def split(frame: np.ndarray, fmt: str = "nv12", depth=None, msb=None):
    """frame (..., 3h/2, w) uint8 (uint16: deep) -> views Y (..., h, w), Cb, Cr (..., h/2, w/2) of the samples AS STORED (words, not
    codes: decode / encode translate).  depth, if given, must agree with the dtype; msb does not change a view."""
    check_fmt(fmt)
    if depth is not None and frame.dtype != container(depth, fmt, msb)[0]:
        raise RuntimeError(f"a {depth}-bit frame is a {np.dtype(container(depth, fmt, msb)[0]).name} array, got {frame.dtype}")
    h, w = frame_size(frame.shape)
    lead = frame.shape[:-2]
    Y = frame[..., :h, :]
    c = frame[..., h:, :]
    if fmt == "i420":
        c = c.reshape(lead + (2, h // 2, w // 2))
        return Y, c[..., 0, :, :], c[..., 1, :, :]
    c = c.reshape(lead + (h // 2, w // 2, 2))
    return (Y, c[..., 0], c[..., 1]) if fmt == "nv12" else (Y, c[..., 1], c[..., 0])


def join(Y: np.ndarray, Cb: np.ndarray, Cr: np.ndarray, fmt: str = "nv12", depth: int = 8, msb=None) -> np.ndarray:
    """The frame of the stored samples Y, Cb, Cr (bytes, or words for a deep frame: the inverse of split)."""
    check_fmt(fmt)
    h, w = Y.shape[-2:]
    out = np.empty(Y.shape[:-2] + frame_shape(h, w), dtype=container(depth, fmt, msb)[0])
    oy, ocb, ocr = split(out, fmt)
    oy[...], ocb[...], ocr[...] = Y, Cb, Cr
    return out


def decode(words: np.ndarray, depth: int, fmt: str = "nv12", msb=None) -> np.ndarray:
    """stored samples -> codes (uint16): word >> shift (MSB-aligned) or min(word, maxcode) (LSB-aligned)."""
    dt, _, maxcode, shift = container(depth, fmt, msb)
    words = np.asarray(words)
    if words.dtype != dt:
        raise RuntimeError(f"a {depth}-bit sample is a {np.dtype(dt).name}, got {words.dtype}")
    return np.minimum(words >> shift, maxcode).astype(np.uint16) if depth > 8 else words


def encode(codes: np.ndarray, depth: int, fmt: str = "nv12", msb=None) -> np.ndarray:
    """codes -> stored samples: code << shift."""
    dt, _, _, shift = container(depth, fmt, msb)
    return (np.asarray(codes).astype(dt) << shift).astype(dt) if depth > 8 else np.asarray(codes).astype(dt)


# ------------------------------------------------------------------------------------------------ the two directions
def _reflect_index(n: int, n_pad: int) -> np.ndarray:
    i = np.arange(n_pad)
    return np.where(i < n, i, 2 * (n - 1) - i)


def ycc_to_rgb(Y, Cb, Cr, to_rgb) -> np.ndarray:
    """Per-sample input expression: uint8 arrays of one shape -> float32 (3,) + shape, clamped to [0, 1]."""
    m = np.asarray(to_rgb, dtype=_F).reshape(3, 4)
    y = Y.astype(_F)
    cb = Cb.astype(_F) - _F(128.0)
    cr = Cr.astype(_F) - _F(128.0)
    out = np.empty((3,) + y.shape, dtype=_F)
    for c in range(3):
        v = ((m[c, 0] * y + m[c, 1] * cb) + m[c, 2] * cr) + m[c, 3]
        out[c] = np.minimum(np.maximum(v, _F(0.0)), _F(1.0))
    return out


def ycc_to_rgb_deep(Y, Cb, Cr, to_rgb, depth: int) -> np.ndarray:
    """The same for n-bit CODES (uint16 arrays of one shape): s = float32(code) * 2^-k, then ycc_to_rgb's expression on s."""
    m = np.asarray(to_rgb, dtype=_F).reshape(3, 4)
    inv = _F(1.0 / (1 << (check_depth(depth) - 8)))
    y = Y.astype(_F) * inv
    cb = Cb.astype(_F) * inv - _F(128.0)
    cr = Cr.astype(_F) * inv - _F(128.0)
    out = np.empty((3,) + y.shape, dtype=_F)
    for c in range(3):
        v = ((m[c, 0] * y + m[c, 1] * cb) + m[c, 2] * cr) + m[c, 3]
        out[c] = np.minimum(np.maximum(v, _F(0.0)), _F(1.0))
    return out


def ycc_to_rgb_sited(y, cb, cr, to_rgb) -> np.ndarray:
    """The same expression on float32 SAMPLES in byte units (float32(code) * 2^-k; cb, cr interpolated by chroma_up, not yet centred)."""
    m = np.asarray(to_rgb, dtype=_F).reshape(3, 4)
    cb, cr = cb - _F(128.0), cr - _F(128.0)
    out = np.empty((3,) + y.shape, dtype=_F)
    for c in range(3):
        v = ((m[c, 0] * y + m[c, 1] * cb) + m[c, 2] * cr) + m[c, 3]
        out[c] = np.minimum(np.maximum(v, _F(0.0)), _F(1.0))
    return out


def chroma_up(C, h: int, w: int, sub, siting: str) -> np.ndarray:
    """Chroma samples C (..., h >> sub_y, w >> sub_x), float32 in byte units, -> the chroma of every source pixel, (..., h, w)
    float32: "Chroma siting, In" of the module docstring.  A centred axis repeats its sample, a co-sited one interpolates."""
    C = np.asarray(C, dtype=_F)
    sub_x, sub_y = sub
    cx, cy = cosited(sub, siting)
    ch, cw = C.shape[-2:]
    if (ch, cw) != (h >> sub_y, w >> sub_x):
        raise RuntimeError(f"a {h}x{w} frame with subsampling {tuple(sub)} has {(h >> sub_y, w >> sub_x)} chroma samples, got {(ch, cw)}")
    sy, sx = np.arange(h), np.arange(w)
    i, j = sy >> sub_y, sx >> sub_x
    i1 = np.minimum(i + (sy & 1), ch - 1) if cy else i
    j1 = np.minimum(j + (sx & 1), cw - 1) if cx else j
    g = lambda a, b: C[..., a, :][..., b]
    return ((g(i, j) + g(i, j1)) + (g(i1, j) + g(i1, j1))) * _F(0.25)


def chroma_down(c, sub, siting: str, offset=0.0) -> np.ndarray:
    """Per-pixel chroma terms c (..., h, w) float32 -> the chroma plane (..., h >> sub_y, w >> sub_x) float32 with `offset` added
    last: "Chroma siting, Out" of the module docstring; the centre rules (box, pair, copy) where no axis is co-sited."""
    c = np.asarray(c, dtype=_F)
    sub_x, sub_y = sub
    cx, cy = cosited(sub, siting)
    off = _F(offset)
    if not sub_x:
        return c + off
    if cx:
        left = np.concatenate([c[..., :, 0:1], c[..., :, 1:-1:2]], axis=-1)              # c[max(2j - 1, 0)]
        t, n = (left + c[..., :, 1::2]) + _F(2.0) * c[..., :, 0::2], 4
    else:
        t, n = c[..., :, 0::2] + c[..., :, 1::2], 2
    if not sub_y:
        return t * _F(1.0 / n) + off
    if cy:
        up = np.concatenate([t[..., 0:1, :], t[..., 1:-1:2, :]], axis=-2)                # t of row max(2i - 1, 0)
        return ((up + t[..., 1::2, :]) + _F(2.0) * t[..., 0::2, :]) * _F(0.25 / n) + off
    return (t[..., 0::2, :] + t[..., 1::2, :]) * _F(0.5 / n) + off


def yuv420_to_planes(frame: np.ndarray, *, fmt: str = "nv12", matrix: str = "bt601", full_range: bool = False, pad=(0, 0), depth: int = 8,
                     msb=None, siting: str = "center") -> np.ndarray:
    """frame (3h/2, w) or (B, 3h/2, w) uint8 (uint16 with depth 10 / 12 / 16) -> (B, 3, h + pad[0], w + pad[1]) float32 RGB planes,
    reflect-padded bottom / right.  siting: "Chroma siting" of the module docstring."""
    if check_siting(siting) != "center":
        check_fmt(fmt)
        return yuv_to_planes(frame, fmt=fmt, matrix=matrix, full_range=full_range, pad=pad, depth=depth, msb=msb, siting=siting)
    frame = np.asarray(frame)
    dt = container(depth, fmt, msb)[0]
    if frame.dtype != dt or frame.ndim not in (2, 3):
        raise RuntimeError(f"expected a (3h/2, w) or (B, 3h/2, w) {np.dtype(dt).name} frame, got {frame.shape} {frame.dtype}")
    if frame.ndim == 2:
        frame = frame[None]
    h, w = frame_size(frame.shape)
    if pad[0] >= h or pad[1] >= w or pad[0] < 0 or pad[1] < 0:
        raise RuntimeError(f"a {h}x{w} frame cannot be reflect-padded by {tuple(pad)}: the padding must be smaller than the frame")
    to_rgb, _ = csc(matrix, full_range, depth)
    Y, Cb, Cr = split(frame, fmt)
    sy, sx = _reflect_index(h, h + pad[0]), _reflect_index(w, w + pad[1])
    Yp = Y[:, sy][:, :, sx]
    Cbp = Cb[:, sy >> 1][:, :, sx >> 1]
    Crp = Cr[:, sy >> 1][:, :, sx >> 1]
    if depth == 8:
        return np.ascontiguousarray(ycc_to_rgb(Yp, Cbp, Crp, to_rgb).transpose(1, 0, 2, 3))
    Yp, Cbp, Crp = (decode(a, depth, fmt, msb) for a in (Yp, Cbp, Crp))
    return np.ascontiguousarray(ycc_to_rgb_deep(Yp, Cbp, Crp, to_rgb, depth).transpose(1, 0, 2, 3))


def _byte(v: np.ndarray) -> np.ndarray:
    return np.rint(np.minimum(np.maximum(v, _F(0.0)), _F(255.0))).astype(np.uint8)


def rgb_to_ycc_float(planes: np.ndarray, from_rgb):
    """planes (..., 3, H, W) float32 -> per-pixel float32 Y (with offset), cb, cr (WITHOUT offset), before any rounding to bytes."""
    k = np.asarray(from_rgb, dtype=_F).reshape(3, 4)
    with np.errstate(invalid="ignore"):
        p = np.minimum(np.maximum(np.asarray(planes, dtype=_F), _F(0.0)), _F(1.0))
    r, g, b = p[..., 0, :, :], p[..., 1, :, :], p[..., 2, :, :]
    Y = ((k[0, 0] * r + k[0, 1] * g) + k[0, 2] * b) + k[0, 3]
    cb = (k[1, 0] * r + k[1, 1] * g) + k[1, 2] * b
    cr = (k[2, 0] * r + k[2, 1] * g) + k[2, 2] * b
    return Y, cb, cr


def _code(v: np.ndarray, k: int, maxcode: int) -> np.ndarray:
    return np.rint(np.minimum(np.maximum(v * _F(1 << k), _F(0.0)), _F(maxcode))).astype(np.uint16)


def planes_to_yuv420(planes: np.ndarray, *, fmt: str = "nv12", matrix: str = "bt601", full_range: bool = False, crop=None, out_depth: int = 8,
                     msb=None, siting: str = "center") -> np.ndarray:
    """planes (B, 3, Hs, Ws) float32 -> (B, 3 h_out / 2, w_out) uint8 (uint16 with out_depth 10 / 12 / 16) in layout `fmt`;
    crop = (h_out, w_out), even, the top-left pixels kept (default: all).  siting: "Chroma siting" of the module docstring."""
    if check_siting(siting) != "center":
        check_fmt(fmt)
        if crop is not None:
            frame_shape(int(crop[0]), int(crop[1]))
        return planes_to_yuv(planes, fmt=fmt, matrix=matrix, full_range=full_range, crop=crop, out_depth=out_depth, msb=msb, siting=siting)
    planes = np.asarray(planes, dtype=_F)
    if planes.ndim != 4 or planes.shape[1] != 3:
        raise RuntimeError(f"expected (B,3,Hs,Ws) float32 planes, got {planes.shape}")
    ho, wo = (planes.shape[2], planes.shape[3]) if crop is None else (int(crop[0]), int(crop[1]))
    frame_shape(ho, wo)
    if ho > planes.shape[2] or wo > planes.shape[3]:
        raise RuntimeError(f"crop {(ho, wo)} does not lie inside the planes {planes.shape[2:]}")
    _, kk, maxcode, _ = container(out_depth, fmt, msb)
    _, k = csc(matrix, full_range, out_depth)
    Y, cb, cr = rgb_to_ycc_float(planes[:, :, :ho, :wo], k)
    box = lambda c, off: ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * _F(0.25) + off
    if out_depth == 8:
        return join(_byte(Y), _byte(box(cb, k[7])), _byte(box(cr, k[11])), fmt)
    q = lambda v: encode(_code(v, kk, maxcode), out_depth, fmt, msb)
    return join(q(Y), q(box(cb, k[7])), q(box(cr, k[11])), fmt, out_depth, msb)


# ------------------------------------------------------------------------------------------------ every subsampling
def check_size(h: int, w: int, fmt: str):
    """(h, w) if an h x w frame exists in layout `fmt`: w even where sub_x = 1, h even where sub_y = 1, both >= 1."""
    sub_x, sub_y, _ = check_layout(fmt)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise RuntimeError(f"a frame has at least one row and one column, got {h}x{w}")
    if sub_x == 1 and w % 2:
        raise RuntimeError(f"{fmt} frames (horizontally subsampled chroma) need an even width, got {h}x{w}")
    if sub_y == 1 and h % 2:
        raise RuntimeError(f"{fmt} frames (vertically subsampled chroma) need an even height, got {h}x{w}")
    return h, w


def _rows(fmt: str):
    """(numerator, denominator) of frame rows per luma row: 3/2, 2, 3 or 1."""
    sub_x, sub_y, _ = check_layout(fmt)
    if sub_x is None:
        return 1, 1
    return {(1, 1): (3, 2), (1, 0): (2, 1), (0, 0): (3, 1)}[(sub_x, sub_y)]


def frame_shape_fmt(h: int, w: int, fmt: str):
    """Shape of the array that holds one h x w frame in layout `fmt`."""
    h, w = check_size(h, w, fmt)
    n, d = _rows(fmt)
    return (n * h // d, w)


def frame_size_fmt(shape, fmt: str):
    """(h, w) of a frame array of layout `fmt` (the shape alone does not name the layout)."""
    n, d = _rows(fmt)
    hh, w = int(shape[-2]), int(shape[-1])
    if hh < 1 or hh % n:
        raise RuntimeError(f"a {fmt} frame is a ({n}h{'/' + str(d) if d > 1 else ''}, w) array, got {tuple(shape)}")
    return check_size(d * hh // n, w, fmt)


def split_fmt(frame: np.ndarray, fmt: str, depth=None, msb=None):
    """frame (..., rows, w) in layout `fmt` -> views Y (..., h, w), Cb, Cr (..., h >> sub_y, w >> sub_x) of the samples as stored;
    Cb and Cr are None for 'gray'."""
    sub_x, sub_y, kind = check_layout(fmt)
    if depth is not None and frame.dtype != container(depth, fmt, msb)[0]:
        raise RuntimeError(f"a {depth}-bit frame is a {np.dtype(container(depth, fmt, msb)[0]).name} array, got {frame.dtype}")
    h, w = frame_size_fmt(frame.shape, fmt)
    if kind == "gray":
        return frame, None, None
    lead, ch, cw = frame.shape[:-2], h >> sub_y, w >> sub_x
    Y, c = frame[..., :h, :], frame[..., h:, :]
    if kind == "planar":
        c = c.reshape(lead + (2, ch, cw))
        return Y, c[..., 0, :, :], c[..., 1, :, :]
    c = c.reshape(lead + (ch, cw, 2))
    return (Y, c[..., 0], c[..., 1]) if kind == "semi" else (Y, c[..., 1], c[..., 0])


def join_fmt(Y: np.ndarray, Cb, Cr, fmt: str, depth: int = 8, msb=None) -> np.ndarray:
    """The frame of the stored samples Y, Cb, Cr in layout `fmt` (the inverse of split_fmt; Cb = Cr = None for 'gray')."""
    h, w = Y.shape[-2:]
    out = np.empty(Y.shape[:-2] + frame_shape_fmt(h, w, fmt), dtype=container(depth, fmt, msb)[0])
    oy, ocb, ocr = split_fmt(out, fmt)
    oy[...] = Y
    if ocb is not None:
        ocb[...], ocr[...] = Cb, Cr
    return out


def yuv_to_planes(frame: np.ndarray, *, fmt: str, matrix: str = "bt601", full_range: bool = False, pad=(0, 0), depth: int = 8,
                  msb=None, siting: str = "center") -> np.ndarray:
    """frame (rows, w) or (B, rows, w) in any layout of LAYOUTS -> (B, 3, h + pad[0], w + pad[1]) float32 RGB planes, reflect-padded
    bottom / right.  yuv420_to_planes for the three 4:2:0 layouts.  siting: "Chroma siting" of the module docstring."""
    frame = np.asarray(frame)
    sub_x, sub_y, kind = check_layout(fmt)
    sited = effective_siting((sub_x, sub_y), siting) != "center"
    dt = container(depth, fmt, msb)[0]
    if frame.dtype != dt or frame.ndim not in (2, 3):
        raise RuntimeError(f"expected a (rows, w) or (B, rows, w) {np.dtype(dt).name} {fmt} frame, got {frame.shape} {frame.dtype}")
    if frame.ndim == 2:
        frame = frame[None]
    h, w = frame_size_fmt(frame.shape, fmt)
    if pad[0] >= h or pad[1] >= w or pad[0] < 0 or pad[1] < 0:
        raise RuntimeError(f"a {h}x{w} frame cannot be reflect-padded by {tuple(pad)}: the padding must be smaller than the frame")
    to_rgb, _ = csc(matrix, full_range, depth)
    Y, Cb, Cr = split_fmt(frame, fmt)
    sy, sx = _reflect_index(h, h + pad[0]), _reflect_index(w, w + pad[1])
    Yp = Y[:, sy][:, :, sx]
    if sited:                # samples in byte units, interpolated per source pixel, then the reflection picks its source pixel
        inv = _F(1.0 / (1 << (depth - 8)))
        val = lambda a: decode(a, depth, fmt, msb).astype(_F) * inv
        Cbp, Crp = (chroma_up(val(a), h, w, (sub_x, sub_y), siting)[:, sy][:, :, sx] for a in (Cb, Cr))
        return np.ascontiguousarray(ycc_to_rgb_sited(val(Yp), Cbp, Crp, to_rgb).transpose(1, 0, 2, 3))
    if kind == "gray":       # Cb' = Cr' = 0: the neutral sample, 128 in byte units at every depth
        Cbp = Crp = np.full(Yp.shape, 128 << (depth - 8), dtype=np.uint16 if depth > 8 else np.uint8)
    else:
        Cbp = Cb[:, sy >> sub_y][:, :, sx >> sub_x]
        Crp = Cr[:, sy >> sub_y][:, :, sx >> sub_x]
    if depth == 8:
        return np.ascontiguousarray(ycc_to_rgb(Yp, Cbp, Crp, to_rgb).transpose(1, 0, 2, 3))
    Yp = decode(Yp, depth, fmt, msb)
    if kind != "gray":
        Cbp, Crp = decode(Cbp, depth, fmt, msb), decode(Crp, depth, fmt, msb)
    return np.ascontiguousarray(ycc_to_rgb_deep(Yp, Cbp, Crp, to_rgb, depth).transpose(1, 0, 2, 3))


def planes_to_yuv(planes: np.ndarray, *, fmt: str, matrix: str = "bt601", full_range: bool = False, crop=None, out_depth: int = 8,
                  msb=None, siting: str = "center") -> np.ndarray:
    """planes (B, 3, Hs, Ws) float32 -> (B,) + frame_shape_fmt(h_out, w_out, fmt) frames in any layout of LAYOUTS; crop = (h_out,
    w_out), the top-left pixels kept (default: all).  planes_to_yuv420 for the three 4:2:0 layouts.  siting: "Chroma siting" of the
    module docstring."""
    planes = np.asarray(planes, dtype=_F)
    sub_x, sub_y, kind = check_layout(fmt)
    sited = effective_siting((sub_x, sub_y), siting) != "center"
    if planes.ndim != 4 or planes.shape[1] != 3:
        raise RuntimeError(f"expected (B,3,Hs,Ws) float32 planes, got {planes.shape}")
    ho, wo = (planes.shape[2], planes.shape[3]) if crop is None else (int(crop[0]), int(crop[1]))
    check_size(ho, wo, fmt)
    if ho > planes.shape[2] or wo > planes.shape[3]:
        raise RuntimeError(f"crop {(ho, wo)} does not lie inside the planes {planes.shape[2:]}")
    _, kk, maxcode, _ = container(out_depth, fmt, msb)
    _, k = csc(matrix, full_range, out_depth)
    Y, cb, cr = rgb_to_ycc_float(planes[:, :, :ho, :wo], k)
    if sited:
        down = lambda c, off: chroma_down(c, (sub_x, sub_y), siting, off)
    elif (sub_x, sub_y) == (1, 1):
        down = lambda c, off: ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * _F(0.25) + off
    elif (sub_x, sub_y) == (1, 0):
        down = lambda c, off: (c[:, :, 0::2] + c[:, :, 1::2]) * _F(0.5) + off
    else:
        down = lambda c, off: c + off
    q = _byte if out_depth == 8 else (lambda v: encode(_code(v, kk, maxcode), out_depth, fmt, msb))
    if kind == "gray":
        return join_fmt(q(Y), None, None, fmt, out_depth, msb)
    return join_fmt(q(Y), q(down(cb, k[7])), q(down(cr, k[11])), fmt, out_depth, msb)


# ------------------------------------------------------------------------------------------------ packed 4:2:2
def check_packed(fmt: str) -> str:
    if fmt not in PACKED_FORMATS:
        raise RuntimeError(f"unknown packed 4:2:2 format {fmt!r}: one of {PACKED_FORMATS}")
    return fmt


def packed_container(fmt: str, depth=None, msb=None):
    """(dtype of the frame array, depth, msb) of packed layout `fmt`: uyvy / yuy2 take depth 8, y210 10 / 12 / 16 (default 10;
    MSB-aligned unless msb=False), v210 10 (its codes are neither: msb is False)."""
    check_packed(fmt)
    if fmt in ("uyvy", "yuy2"):
        want, dt = (8,), np.uint8
    elif fmt == "y210":
        want, dt = (10, 12, 16), np.uint16
    else:
        want, dt = (10,), np.uint8
    depth = want[0] if depth is None else depth
    if isinstance(depth, bool) or depth not in want:
        raise RuntimeError(f"{fmt} frames hold {' / '.join(map(str, want))}-bit samples, not depth {depth!r}")
    return dt, int(depth), (True if msb is None else bool(msb)) if fmt == "y210" else False


def _check_packed_size(h, w, fmt):
    h, w = int(h), int(w)
    if h < 1 or w < 2 or w % 2:
        raise RuntimeError(f"{fmt} frames (packed 4:2:2) need an even width >= 2 and at least one row, got {h}x{w}")
    return h, w


def packed_shape(h: int, w: int, fmt: str):
    """Shape of the array that holds one h x w frame in packed layout `fmt`."""
    check_packed(fmt)
    h, w = _check_packed_size(h, w, fmt)
    return (h, 128 * -(-w // 48)) if fmt == "v210" else (h, 2 * w)


def packed_size(shape, fmt: str, width=None):
    """(h, w) of a packed frame array; width is required for v210 (the row length does not give it), optional and checked otherwise."""
    check_packed(fmt)
    h, cols = int(shape[-2]), int(shape[-1])
    if fmt == "v210":
        if width is None:
            raise ValueError("a v210 frame does not give its width (a row is 128 ceil(w / 48) bytes): pass width=")
        w = int(width)
    else:
        w = cols // 2
        if width is not None and int(width) != w:
            raise ValueError(f"width={width} does not agree with a {fmt} frame of {tuple(shape)}: its rows hold {w} pixels")
    if cols < 1 or packed_shape(h, w, fmt) != (h, cols):
        raise RuntimeError(f"a {h}x{w} {fmt} frame is a {packed_shape(h, w, fmt) if w >= 2 and not w % 2 and h >= 1 else '(h, row)'} array, got {tuple(shape)}")
    return h, w


_V210_WORD = np.arange(12) // 3           # component n of a group (Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 Cb2 Y4 Cr2 Y5) lies in this word
_V210_SHIFT = 10 * (np.arange(12) % 3)    # at this bit


def unpack422(frame: np.ndarray, fmt: str, w: int, depth=None, msb=None):
    """frame (..., h, row) in packed layout `fmt` -> Y (..., h, w), Cb, Cr (..., h, w / 2): the samples AS STORED (bytes; y210: words
    in their alignment, what decode reads with the same depth and msb; v210: the 10-bit codes as uint16)."""
    dt, depth, msb = packed_container(fmt, depth, msb)
    frame = np.asarray(frame)
    if frame.dtype != dt or frame.ndim < 2:
        raise RuntimeError(f"a {fmt} frame is a (h, row) {np.dtype(dt).name} array, got {frame.shape} {frame.dtype}")
    h, w = packed_size(frame.shape, fmt, w)
    if fmt != "v210":
        q = frame.reshape(frame.shape[:-1] + (w // 2, 4))
        iy0, icb, iy1, icr = (1, 0, 3, 2) if fmt == "uyvy" else (0, 1, 2, 3)
        Y = np.stack([q[..., iy0], q[..., iy1]], axis=-1).reshape(frame.shape[:-1] + (w,))
        return Y, q[..., icb].copy(), q[..., icr].copy()
    g = -(-w // 6)
    words = np.ascontiguousarray(frame[..., :16 * g]).view("<u4").reshape(frame.shape[:-1] + (g, 4))
    comp = ((words[..., _V210_WORD] >> _V210_SHIFT.astype(np.uint32)) & np.uint32(1023)).astype(np.uint16)   # (..., g, 12)
    lead = frame.shape[:-1]
    Y = comp[..., 1::2].reshape(lead + (6 * g,))[..., :w]
    Cb = comp[..., 0::4].reshape(lead + (3 * g,))[..., :w // 2]
    Cr = comp[..., 2::4].reshape(lead + (3 * g,))[..., :w // 2]
    return np.ascontiguousarray(Y), np.ascontiguousarray(Cb), np.ascontiguousarray(Cr)


def pack422(Y: np.ndarray, Cb: np.ndarray, Cr: np.ndarray, fmt: str, depth=None, msb=None) -> np.ndarray:
    """The packed frame of the stored samples Y (..., h, w), Cb, Cr (..., h, w / 2): the inverse of unpack422 (v210: of 10-bit codes;
    the top bits, the codes past w and the row tail are zero)."""
    dt, depth, msb = packed_container(fmt, depth, msb)
    Y, Cb, Cr = np.asarray(Y), np.asarray(Cb), np.asarray(Cr)
    h, w = Y.shape[-2:]
    lead = Y.shape[:-2]
    shape = packed_shape(h, w, fmt)
    if Cb.shape != lead + (h, w // 2) or Cr.shape != Cb.shape:
        raise RuntimeError(f"a {h}x{w} 4:2:2 frame has ({h}, {w // 2}) chroma samples a plane, got {Cb.shape[-2:]} / {Cr.shape[-2:]}")
    if fmt != "v210":
        out = np.empty(lead + (h, w // 2, 4), dtype=dt)
        iy0, icb, iy1, icr = (1, 0, 3, 2) if fmt == "uyvy" else (0, 1, 2, 3)
        out[..., iy0], out[..., iy1], out[..., icb], out[..., icr] = Y[..., 0::2], Y[..., 1::2], Cb, Cr
        return out.reshape(lead + shape)
    g = -(-w // 6)
    comp = np.zeros(lead + (h, g, 12), dtype=np.uint32)
    fill = lambda a, n: np.concatenate([a.astype(np.uint32) & np.uint32(1023), np.zeros(lead + (h, n - a.shape[-1]), np.uint32)], axis=-1)
    comp[..., 1::2] = fill(Y, 6 * g).reshape(lead + (h, g, 6))
    comp[..., 0::4] = fill(Cb, 3 * g).reshape(lead + (h, g, 3))
    comp[..., 2::4] = fill(Cr, 3 * g).reshape(lead + (h, g, 3))
    words = np.zeros(lead + (h, g, 4), dtype=np.uint32)
    for n in range(12):
        words[..., _V210_WORD[n]] |= comp[..., n] << np.uint32(_V210_SHIFT[n])
    out = np.zeros(lead + shape, dtype=np.uint8)
    out[..., :16 * g] = words.astype("<u4").reshape(lead + (h, 4 * g)).view(np.uint8)
    return out


def packed_to_planes(frame: np.ndarray, *, fmt: str, width=None, matrix: str = "bt601", full_range: bool = False, pad=(0, 0), depth=None,
                     msb=None, siting: str = "center") -> np.ndarray:
    """frame (h, row) or (B, h, row) in packed 4:2:2 layout `fmt` -> (B, 3, h + pad[0], w + pad[1]) float32 RGB planes: yuv_to_planes of
    the 'i422' frame with the same samples ("Packed 4:2:2" of the module docstring).  siting 'center' (the default) or 'left' ('topleft'
    means 'left'); standard 4:2:2 video is left-sited."""
    _, depth, msb = packed_container(fmt, depth, msb)
    frame = np.asarray(frame)
    if frame.ndim not in (2, 3):
        raise RuntimeError(f"expected a (h, row) or (B, h, row) {fmt} frame, got {frame.shape}")
    w = packed_size(frame.shape, fmt, width)[1]
    planar = join_fmt(*unpack422(frame, fmt, w, depth, msb), "i422", depth, msb)
    return yuv_to_planes(planar, fmt="i422", matrix=matrix, full_range=full_range, pad=pad, depth=depth, msb=msb, siting=siting)


def planes_to_packed(planes: np.ndarray, *, fmt: str, matrix: str = "bt601", full_range: bool = False, crop=None, out_depth=None, msb=None,
                     siting: str = "center") -> np.ndarray:
    """planes (B, 3, Hs, Ws) float32 -> (B,) + packed_shape(h_out, w_out, fmt) frames in packed 4:2:2 layout `fmt`: pack422 of the samples
    of planes_to_yuv(fmt='i422'); crop = (h_out, w_out), w_out even (default: all).  siting: as packed_to_planes."""
    _, depth, msb = packed_container(fmt, out_depth, msb)
    planes = np.asarray(planes, dtype=_F)
    if planes.ndim == 4:
        _check_packed_size(*((planes.shape[2], planes.shape[3]) if crop is None else crop), fmt)
    planar = planes_to_yuv(planes, fmt="i422", matrix=matrix, full_range=full_range, crop=crop, out_depth=depth, msb=msb, siting=siting)
    return pack422(*split_fmt(planar, "i422"), fmt, depth, msb)
