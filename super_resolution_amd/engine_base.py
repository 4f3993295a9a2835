"""`EngineBase` — the run-time state HATEngine and ESCEngine share: the device and compute dtype, the lock and device guard around
a forward, and the per-shape workspace LRU.  What a network is (packing, workspace layout, launches) is the subclass's.  DESIGN.md §4."""
from __future__ import annotations

import collections
import os
import threading

import torch

from . import ops


class EngineBase:
    """A subclass implements `_forward(x, **kw)`, the launches of one forward, and `_alloc_workspace(B, H, W, tag)`, the dict of
    zero-filled device buffers one input shape needs."""

    def __init__(self, device, dtype: str, ws_max: int):
        self.dev = torch.device(device)
        self.dtype = ops.DTYPE_CODE[dtype]
        self.tdt = ops.TORCH_DTYPE[self.dtype]
        self._lock = threading.Lock()   # one forward at a time per engine: the workspace and side stream are shared state
        # per-shape workspaces, least recently used first; tiled inference alternates between a few shapes (interior /
        # edge / corner tiles), so a small LRU (at most ws_max entries and HAT_WS_CACHE_GIB bytes) allocates and zero-fills each once
        self._ws_cache = collections.OrderedDict()
        self._ws_max, self._ws_max_bytes = ws_max, int(float(os.environ.get("HAT_WS_CACHE_GIB", "96")) * 2 ** 30)
        self.ws_allocations = 0

    def forward(self, x: torch.Tensor, **kw) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("HAT forward needs a device tensor: the HIP path is the only path")
        if x.device != self.dev:
            raise RuntimeError(f"input is on {x.device} but this engine's weights and workspace live on {self.dev}")
        # kernels are enqueued on the CURRENT stream of the engine's device: make that device current for the launches
        # (the C side never switches devices), and serialise callers: workspace and side stream are per-engine state
        with self._lock, torch.cuda.device(self.dev):
            return self._forward(x, **kw)

    def _workspace(self, B, H, W, tag=None):
        """tag: a row band of a sharded frame gets a workspace of its own (two bands of one shape must not share buffers)."""
        key = (B, H, W) if tag is None else (B, H, W, tag)
        w = self._ws_cache.get(key)
        if w is not None:
            self._ws_cache.move_to_end(key)
            return w
        w = self._alloc_workspace(B, H, W, tag)
        w["bytes"] = sum(t.numel() * t.element_size() for v in w.values() for t in (v if isinstance(v, list) else [v])
                         if isinstance(t, torch.Tensor))
        self._ws_cache[key] = w
        self.ws_allocations += 1
        while len(self._ws_cache) > 1 and (len(self._ws_cache) > self._ws_max
                                           or sum(v["bytes"] for v in self._ws_cache.values()) > self._ws_max_bytes):
            self._ws_cache.popitem(last=False)   # graphs captured on an evicted workspace keep their own reference
        return w
