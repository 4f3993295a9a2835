"""YUV4MPEG2 (.y4m) files of 8-bit 4:2:0 video: a reader and a writer, nothing else.

A stream is one header line `YUV4MPEG2 W<w> H<h> F<num>:<den> I<p|t|b|m> A<n>:<d> C<colour space> [X...]` and, per frame,
a line `FRAME[ params]` followed by the planes Y (h x w), Cb, Cr (h/2 x w/2 each): that is the 'i420' layout of yuv.py,
so a frame is a (3h/2, w) uint8 array.  Accepted colour spaces: C420 (the default when the token is absent), C420jpeg,
C420mpeg2, C420paldv — they differ in chroma siting only, which this project treats alike (yuv.py).  Every other colour
space (C444, C422, Cmono ...), more than 8 bits (C420p10 ...) and odd sizes are refused by name.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"YUV4MPEG2"
COLOUR_SPACES = ("420", "420jpeg", "420mpeg2", "420paldv")
TOKENS = "WHFIAC"


class Y4MError(RuntimeError):
    pass


def parse_header(line: bytes) -> dict:
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
    if c not in COLOUR_SPACES:
        if c.startswith("420p"):
            raise Y4MError(f"colour space C{c} has more than 8 bits per sample: only 8-bit 4:2:0 is supported")
        raise Y4MError(f"colour space C{c} is not supported: only 8-bit 4:2:0 (C420, C420jpeg, C420mpeg2, C420paldv)")
    if hdr["W"] % 2 or hdr["H"] % 2:
        raise Y4MError(f"4:2:0 frames need even sizes, got W{hdr['W']} H{hdr['H']}")
    return hdr


def format_header(hdr: dict) -> bytes:
    """The header line for W, H and whichever of F, I, A, C, X are present, in that order, with its newline."""
    parse_header(b" ".join([MAGIC, b"W%d" % hdr["W"], b"H%d" % hdr["H"]] + ([b"C" + hdr["C"].encode()] if "C" in hdr else [])))
    out = [MAGIC, b"W%d" % hdr["W"], b"H%d" % hdr["H"]]
    out += [k.encode() + str(hdr[k]).encode() for k in "FIAC" if k in hdr]
    out += [b"X" + x.encode() for x in hdr.get("X", [])]
    return b" ".join(out) + b"\n"


def scaled_header(hdr: dict, scale: int) -> dict:
    """The header of the upscaled stream: W and H multiplied by the scale, every other token copied."""
    return dict(hdr, W=hdr["W"] * scale, H=hdr["H"] * scale, X=list(hdr.get("X", [])))


def _readline(f, limit: int = 4096) -> bytes:
    line = f.readline(limit)
    if len(line) == limit and not line.endswith(b"\n"):
        raise Y4MError("a header line is longer than 4096 bytes")
    return line


class Reader:
    """Iterates the frames of a .y4m file as (3h/2, w) uint8 arrays (layout 'i420'); .header is the parsed header."""

    def __init__(self, path_or_file):
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "rb") if self._own else path_or_file
        line = _readline(self._f)
        if not line.endswith(b"\n"):
            self.close()
            raise Y4MError("the stream ends inside its header")
        try:
            self.header = parse_header(line[:-1])
        except Y4MError:
            self.close()
            raise
        self.w, self.h = self.header["W"], self.header["H"]

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        line = _readline(self._f)
        if not line:
            raise StopIteration
        if not line.endswith(b"\n") or not (line == b"FRAME\n" or line.startswith(b"FRAME ")):
            raise Y4MError(f"expected a FRAME record, got {line[:16]!r}")
        n = self.w * self.h * 3 // 2
        raw = self._f.read(n)
        if len(raw) != n:
            raise Y4MError(f"truncated frame: {len(raw)} of {n} bytes")
        return np.frombuffer(raw, dtype=np.uint8).reshape(3 * self.h // 2, self.w)

    def close(self):
        if self._own and self._f:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Writer:
    """Writes (3h/2, w) uint8 'i420' frames as a .y4m file with the given header (a dict as parse_header returns)."""

    def __init__(self, path_or_file, header: dict):
        self.header = dict(header)
        head = format_header(self.header)
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        self._shape = (3 * header["H"] // 2, header["W"])
        self._f.write(head)

    def write(self, frame: np.ndarray):
        frame = np.ascontiguousarray(frame)
        if frame.shape != self._shape or frame.dtype != np.uint8:
            raise Y4MError(f"a frame of this stream is a {self._shape} uint8 array, got {frame.shape} {frame.dtype}")
        self._f.write(b"FRAME\n")
        self._f.write(frame.tobytes())

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
