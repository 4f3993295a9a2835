"""Headerless files of packed 4:2:2 frames (`ffmpeg -f rawvideo -pix_fmt uyvy422 | yuyv422 | y210le | v210`): frame after frame, each
yuv.packed_shape(h, w, fmt) samples, little-endian, nothing between them.  The file says neither its size nor its layout: the
caller does.  No threads, no dependencies beyond numpy."""
from __future__ import annotations

import numpy as np

from . import yuv


class RawVideoError(RuntimeError):
    pass


class _File:
    def __init__(self, path_or_file, mode: str, fmt: str, h: int, w: int, depth=None):
        self.fmt = yuv.check_packed(fmt)
        dt, self.depth, _ = yuv.packed_container(fmt, depth)
        self.h, self.w = int(h), int(w)
        self._shape = yuv.packed_shape(h, w, fmt)
        self._dtype = np.dtype(dt).newbyteorder("<") if np.dtype(dt).itemsize > 1 else np.dtype(dt)
        self.frame_bytes = self._shape[0] * self._shape[1] * self._dtype.itemsize
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, mode) if self._own else path_or_file

    def close(self):
        if self._f:
            if "w" in getattr(self._f, "mode", "") or not self._own:
                try:
                    self._f.flush()
                except (ValueError, OSError):
                    pass
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Reader(_File):
    """Iterates the frames of a headerless file as yuv.packed_shape(h, w, fmt) arrays: uint8 (uyvy, yuy2, v210) or uint16 (y210, depth 10 /
    12 / 16).  A file that ends inside a frame is an error."""

    def __init__(self, path_or_file, fmt: str, h: int, w: int, depth=None):
        super().__init__(path_or_file, "rb", fmt, h, w, depth)

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        raw = self._f.read(self.frame_bytes)
        if not raw:
            raise StopIteration
        if len(raw) != self.frame_bytes:
            raise RawVideoError(f"truncated frame: {len(raw)} of {self.frame_bytes} bytes ({self.h}x{self.w} {self.fmt})")
        return np.frombuffer(raw, dtype=self._dtype).reshape(self._shape).astype(self._dtype.newbyteorder("="), copy=False)


class Writer(_File):
    """Writes yuv.packed_shape(h, w, fmt) frames to a headerless file, 16-bit words little-endian."""

    def __init__(self, path_or_file, fmt: str, h: int, w: int, depth=None):
        super().__init__(path_or_file, "wb", fmt, h, w, depth)

    def write(self, frame: np.ndarray):
        frame = np.ascontiguousarray(frame)
        if frame.shape != self._shape or frame.dtype.itemsize != self._dtype.itemsize or frame.dtype.kind != "u":
            raise RawVideoError(f"a frame of this file is a {self._shape} {self._dtype.name} array, got {frame.shape} {frame.dtype}")
        self._f.write(frame.astype(self._dtype, copy=False).tobytes())
