"""YUV4MPEG2 (.y4m) files of 4:2:0 video, 8-bit and (with deep=True) 10 / 12 / 16-bit: a reader and a writer, nothing else.

A stream is one header line `YUV4MPEG2 W<w> H<h> F<num>:<den> I<p|t|b|m> A<n>:<d> C<colour space> [X...]` and, per frame,
a line `FRAME[ params]` followed by the planes Y (h x w), Cb, Cr (h/2 x w/2 each): that is the 'i420' layout of yuv.py,
so a frame is a (3h/2, w) uint8 array.  Accepted colour spaces: C420 (the default when the token is absent), C420jpeg,
C420mpeg2, C420paldv — they differ in chroma siting only: the reader hands over the same arrays, siting_of(hdr) names the
siting ('center', 'left', 'topleft': yuv.py, "Chroma siting") and with_siting(hdr, siting) writes it back.  Every other colour
space (C444, C422, Cmono ...), more than 8 bits (C420p10 ...) and odd sizes are refused by name.

deep=True (parse_header, Reader, Writer) also accepts C420p10, C420p12 and C420p16: every sample is a little-endian 16-bit word
holding the code LSB-aligned (yuv.py, "Deep samples"), a frame is a (3h/2, w) uint16 array and its record is 3 w h bytes long.
depth(hdr) is 8, 10, 12 or 16.  Without deep=True these streams are refused as before.

chroma=True (parse_header, format_header, Reader, Writer; it includes deep=True) also accepts C422, C444 and Cmono and their deep
forms C422p10 / p12 / p16, C444p10 / p12 / p16, Cmono10 / Cmono12 / Cmono16.  Reader.fmt / Writer.fmt names the layout of yuv.py
('i420', 'i422', 'i444' or 'gray'), a frame is an array of yuv.frame_shape_fmt(h, w, fmt) and its record holds 3/2, 2, 3 or 1
times w h samples; only the subsampled directions need even sizes.  chroma(hdr) is '420', '422', '444' or 'mono';
with_chroma(hdr, c) rewrites the C token.  C444alpha and everything else is still refused by name.  Without chroma=True the
behaviour is what it was.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"YUV4MPEG2"
COLOUR_SPACES = ("420", "420jpeg", "420mpeg2", "420paldv")
DEEP_COLOUR_SPACES = {"420p10": 10, "420p12": 12, "420p16": 16}
TOKENS = "WHFIAC"
CHROMAS = {"420": "i420", "422": "i422", "444": "i444", "mono": "gray"}   # chroma(hdr) -> layout of yuv.py
_CHROMA_SPACES = {}   # C token (chroma=True) -> (chroma, bits)
for _c in ("422", "444"):
    _CHROMA_SPACES[_c] = (_c, 8)
    for _b in (10, 12, 16):
        _CHROMA_SPACES[f"{_c}p{_b}"] = (_c, _b)
_CHROMA_SPACES["mono"] = ("mono", 8)
for _b in (10, 12, 16):
    _CHROMA_SPACES[f"mono{_b}"] = ("mono", _b)


class Y4MError(RuntimeError):
    pass


_SITING_OF_TOKEN = {"420jpeg": "center", "420mpeg2": "left", "420paldv": "topleft"}
_TOKEN_OF_SITING = {v: k for k, v in _SITING_OF_TOKEN.items()}
_XYSCSS = "YSCSS="     # the X comment `XYSCSS=<name>` as parse_header keeps it (without its X): ffmpeg / mjpegtools' extension


def siting_of(hdr: dict) -> str:
    """The chroma siting (yuv.SITINGS) a header names: C420mpeg2 -> 'left', C420paldv -> 'topleft' (its alternating-line detail
    is out of scope), C420jpeg -> 'center'.  A bare C420 and every token without a siting (C420p10, C422*, C444*, Cmono*) is
    'center' unless an XYSCSS=420MPEG2 | 420PALDV | 420JPEG comment says otherwise (the last such comment counts).  A 4:2:2 header
    cannot say: standard 4:2:2 is 'left', and the caller asks for it."""
    c = hdr.get("C", "420")
    if c in ("420mpeg2", "420paldv"):
        return _SITING_OF_TOKEN[c]
    for x in reversed(hdr.get("X", [])):
        if x.startswith(_XYSCSS) and x[len(_XYSCSS):].lower() in _SITING_OF_TOKEN:
            return _SITING_OF_TOKEN[x[len(_XYSCSS):].lower()]
    return "center"


def with_siting(hdr: dict, siting: str) -> dict:
    """The header saying `siting`: an 8-bit 4:2:0 C token becomes C420jpeg / C420mpeg2 / C420paldv (a bare C420 stays bare for
    'center'), and an XYSCSS=420* comment that is there is rewritten to agree.  Tokens that cannot carry a siting (deep 4:2:0
    without an XYSCSS comment, 4:2:2, 4:4:4, mono) are left alone."""
    if siting not in _TOKEN_OF_SITING:
        raise Y4MError(f"unknown chroma siting {siting!r}: one of {tuple(_TOKEN_OF_SITING)}")
    out = dict(hdr, X=list(hdr.get("X", [])))
    c = hdr.get("C", "420")
    if c in _SITING_OF_TOKEN or (c == "420" and siting != "center"):
        out["C"] = _TOKEN_OF_SITING[siting]
    if chroma(hdr) == "420":
        out["X"] = [_XYSCSS + _TOKEN_OF_SITING[siting].upper() if x.startswith(_XYSCSS + "420") else x for x in out["X"]]
    return out


def depth(hdr: dict) -> int:
    """Bits per sample of a stream with this header: 8, or 10 / 12 / 16 for C420p10 / C420p12 / C420p16."""
    c = hdr.get("C", "420")
    return _CHROMA_SPACES[c][1] if c in _CHROMA_SPACES else DEEP_COLOUR_SPACES.get(c, 8)


def chroma(hdr: dict) -> str:
    """'420', '422', '444' or 'mono': the subsampling the header's C token names (CHROMAS maps it to a layout of yuv.py)."""
    c = hdr.get("C", "420")
    return _CHROMA_SPACES[c][0] if c in _CHROMA_SPACES else "420"


_chroma_of = chroma    # (parse_header, Reader and Writer take a keyword of this name)


def with_chroma(hdr: dict, c: str, bits=None) -> dict:
    """The header with its C token set for subsampling `c` ('420', '422', '444', 'mono') at `bits` per sample (default: the
    header's); a token that already says so is kept (C420jpeg stays C420jpeg)."""
    if c not in CHROMAS:
        raise Y4MError(f"unknown chroma subsampling {c!r}: one of {tuple(CHROMAS)}")
    bits = depth(hdr) if bits is None else bits
    if bits not in (8, 10, 12, 16):
        raise Y4MError(f"a stream has 8, 10, 12 or 16 bits per sample, got {bits}")
    if c == chroma(hdr) and bits == depth(hdr):
        return dict(hdr)
    return dict(hdr, C=c if bits == 8 else (f"mono{bits}" if c == "mono" else f"{c}p{bits}"))


def with_depth(hdr: dict, bits: int) -> dict:
    """The header with its C token set for `bits` per sample: an 8-bit token is kept, a change of width writes C420 / C420p<bits>."""
    if bits not in (8, 10, 12, 16):
        raise Y4MError(f"a 4:2:0 stream has 8, 10, 12 or 16 bits per sample, got {bits}")
    if bits == depth(hdr):
        return dict(hdr)
    if chroma(hdr) != "420":
        return with_chroma(hdr, chroma(hdr), bits)
    return dict(hdr, C="420" if bits == 8 else f"420p{bits}")


def parse_header(line: bytes, deep: bool = False, chroma: bool = False) -> dict:
    """The header line (without its newline) -> {'W': int, 'H': int, 'F': str, 'I': str, 'A': str, 'C': str, 'X': [str ...]};
    tokens that are absent are absent (C defaults to '420' for the reader's purposes)."""
    parts = line.split(b" ")
    if not parts or parts[0] != MAGIC:
        raise Y4MError("not a YUV4MPEG2 stream (the header does not start with 'YUV4MPEG2')")
    hdr: dict = {"X": []}
    for tok in parts[1:]:
        if not tok:
            continue
        t = tok.decode("ascii", "replace")
        key, val = t[0], t[1:]
        if key == "X":
            hdr["X"].append(val)
        elif key in "WH":
            if not val.isdigit() or int(val) < 1:
                raise Y4MError(f"bad {key} token {t!r}")
            hdr[key] = int(val)
        elif key in TOKENS:
            hdr[key] = val
        else:
            raise Y4MError(f"unknown header token {t!r}")
    if "W" not in hdr or "H" not in hdr:
        raise Y4MError("the header names no W / H")
    c = hdr.get("C", "420")
    if chroma:
        if c in _CHROMA_SPACES:
            sub = _CHROMA_SPACES[c][0]
            if sub == "422" and hdr["W"] % 2:
                raise Y4MError(f"4:2:2 frames need an even width, got W{hdr['W']} H{hdr['H']}")
            return hdr
        if c not in COLOUR_SPACES and c not in DEEP_COLOUR_SPACES:
            raise Y4MError(f"colour space C{c} is not supported: C420 (jpeg, mpeg2, paldv), C422, C444, Cmono and their 10 / 12 / 16-bit forms")
        deep = True
    if c not in COLOUR_SPACES and not (deep and c in DEEP_COLOUR_SPACES):
        if c.startswith("420p"):
            raise Y4MError(f"colour space C{c} has more than 8 bits per sample: only 8-bit 4:2:0 is supported")
        raise Y4MError(f"colour space C{c} is not supported: only 8-bit 4:2:0 (C420, C420jpeg, C420mpeg2, C420paldv)")
    if hdr["W"] % 2 or hdr["H"] % 2:
        raise Y4MError(f"4:2:0 frames need even sizes, got W{hdr['W']} H{hdr['H']}")
    return hdr


def format_header(hdr: dict, deep: bool = False, chroma: bool = False) -> bytes:
    """The header line for W, H and whichever of F, I, A, C, X are present, in that order, with its newline."""
    parse_header(b" ".join([MAGIC, b"W%d" % hdr["W"], b"H%d" % hdr["H"]] + ([b"C" + hdr["C"].encode()] if "C" in hdr else [])), deep, chroma)
    out = [MAGIC, b"W%d" % hdr["W"], b"H%d" % hdr["H"]]
    out += [k.encode() + str(hdr[k]).encode() for k in "FIAC" if k in hdr]
    out += [b"X" + x.encode() for x in hdr.get("X", [])]
    return b" ".join(out) + b"\n"


def scaled_header(hdr: dict, scale: int) -> dict:
    """The header of the upscaled stream: W and H multiplied by the scale, every other token copied."""
    return dict(hdr, W=hdr["W"] * scale, H=hdr["H"] * scale, X=list(hdr.get("X", [])))


def sized_header(hdr: dict, w: int, h: int) -> dict:
    """The header of a stream resized to w x h (an arbitrary-scale network's output): W and H set, every other token copied.  The
    pixel aspect ratio `A` is copied as it is even where the two axes are scaled by different factors: the caller chose the size,
    and whether the pixels or the picture keep their shape is the caller's to say."""
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise Y4MError(f"a stream of {w}x{h} is empty")
    return dict(hdr, W=w, H=h, X=list(hdr.get("X", [])))


def _readline(f, limit: int = 4096) -> bytes:
    line = f.readline(limit)
    if len(line) == limit and not line.endswith(b"\n"):
        raise Y4MError("a header line is longer than 4096 bytes")
    return line


def _frame_shape(h: int, w: int, fmt: str):
    return {"i420": (3 * h // 2, w), "i422": (2 * h, w), "i444": (3 * h, w), "gray": (h, w)}[fmt]


class Reader:
    """Iterates the frames of a .y4m file as (3h/2, w) uint8 arrays (layout 'i420'); .header is the parsed header.  deep=True:
    C420p10 / p12 / p16 streams are read too, as uint16 arrays (.depth says which)."""

    def __init__(self, path_or_file, deep: bool = False, chroma: bool = False):
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "rb") if self._own else path_or_file
        line = _readline(self._f)
        if not line.endswith(b"\n"):
            self.close()
            raise Y4MError("the stream ends inside its header")
        try:
            self.header = parse_header(line[:-1], deep, chroma)
        except Y4MError:
            self.close()
            raise
        self.w, self.h = self.header["W"], self.header["H"]
        self.depth = depth(self.header)
        self._dtype = np.dtype(np.uint8) if self.depth == 8 else np.dtype("<u2")
        self.fmt = CHROMAS[_chroma_of(self.header)]      # 'i420' unless chroma=True let another colour space in
        self._shape = _frame_shape(self.h, self.w, self.fmt)

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        line = _readline(self._f)
        if not line:
            raise StopIteration
        if not line.endswith(b"\n") or not (line == b"FRAME\n" or line.startswith(b"FRAME ")):
            raise Y4MError(f"expected a FRAME record, got {line[:16]!r}")
        n = self._shape[0] * self._shape[1] * self._dtype.itemsize
        raw = self._f.read(n)
        if len(raw) != n:
            raise Y4MError(f"truncated frame: {len(raw)} of {n} bytes")
        return np.frombuffer(raw, dtype=self._dtype).reshape(self._shape)

    def close(self):
        if self._own and self._f:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Writer:
    """Writes (3h/2, w) uint8 'i420' frames as a .y4m file with the given header (a dict as parse_header returns).  deep=True:
    a C420p10 / p12 / p16 header is accepted and its frames are uint16 arrays, written as little-endian words."""

    def __init__(self, path_or_file, header: dict, deep: bool = False, chroma: bool = False):
        self.header = dict(header)
        head = format_header(self.header, deep, chroma)
        self.fmt = CHROMAS[_chroma_of(self.header)]
        self._dtype = np.dtype(np.uint8) if depth(self.header) == 8 else np.dtype(np.uint16)
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        self._shape = _frame_shape(header["H"], header["W"], self.fmt)
        self._f.write(head)

    def write(self, frame: np.ndarray):
        frame = np.ascontiguousarray(frame)
        if frame.shape != self._shape or frame.dtype != self._dtype:
            raise Y4MError(f"a frame of this stream is a {self._shape} {self._dtype.name} array, got {frame.shape} {frame.dtype}")
        self._f.write(b"FRAME\n")
        self._f.write(frame.tobytes() if self._dtype.itemsize == 1 else frame.astype("<u2", copy=False).tobytes())

    def close(self):
        if self._f:
            self._f.flush()
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
