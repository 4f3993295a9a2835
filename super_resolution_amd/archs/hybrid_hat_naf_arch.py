"""`HybridHATNAF` — drop-in for the reference's `hat.archs.hybrid_hat_naf_arch.HybridHATNAF` (hybrid_hat_naf_arch.py:85-136):
a NAFNet-style stem at LR size, x_naf = x + tail(body(head(x))), whose output feeds an unchanged `HATX`.

Same constructor keywords and merge rules (:109-118), same attributes (`window_size`, `upscale`, `in_chans`, `img_range`), same
`state_dict()` surface: `naf.head.*`, `naf.body.{i}.{beta,gamma,pw1,dw,sca.1,pw2,ffn1,ffn_dw,ffn2}.*`, `naf.tail.*`, then the
whole HATX surface under `hat.`.  Like `HAT`, the module tree only holds parameters: the forward hands them to `HATEngine`,
which runs the stem (hat_naf_half / hat_naf_fold, include/hat_mi355x.h "NAF stem") in front of HATX's own launch sequence.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .hat_arch import HAT, HATX, _Holder


class _NAFBlock(_Holder):  # hybrid_hat_naf_arch.py:16-48
    def __init__(self, c, dw_expand=2, ffn_expand=2):
        super().__init__()
        dwc, ffnc = c * dw_expand, c * ffn_expand
        self.pw1 = nn.Conv2d(c, dwc, 1, 1, 0)
        self.dw = nn.Conv2d(dwc, dwc, 3, 1, 1, groups=dwc)
        self.sca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(dwc // 2, dwc // 2, 1, 1, 0))
        self.pw2 = nn.Conv2d(dwc // 2, c, 1, 1, 0)
        self.ffn1 = nn.Conv2d(c, ffnc, 1, 1, 0)
        self.ffn_dw = nn.Conv2d(ffnc, ffnc, 3, 1, 1, groups=ffnc)
        self.ffn2 = nn.Conv2d(ffnc // 2, c, 1, 1, 0)
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)))
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)))


class _NAFStem(_Holder):  # hybrid_hat_naf_arch.py:69-75
    def __init__(self, in_ch=3, width=64, n_blocks=4):
        super().__init__()
        self.head = nn.Conv2d(in_ch, width, 3, 1, 1)
        self.body = nn.Sequential(*[_NAFBlock(width) for _ in range(n_blocks)])
        self.tail = nn.Conv2d(width, in_ch, 3, 1, 1)


@ARCH_REGISTRY.register()
class HybridHATNAF(HAT):
    """x --(NAF stem)--> x_naf --(HATX)--> y on the MI355X.  It is a `HAT` from the engine up — `compute_dtype` /
    `set_compute_dtype`, `use_graph`, the weight-change tracking and every `forward*` method are HAT's own — over a module tree
    of its own: `naf` and a `HATX` under `hat`, whose parameters the engine packs together.

    `naf_width` 64 (the default) and 32 are built; any other width, and an `in_chans` other than 3, is a ValueError when the engine
    packs.  `forward_bands` / `forward_band_parallel` raise NotImplementedError.  Extra (non-reference) keywords:
    `compute_dtype` ('bf16' | 'f32'; default: hat_kwargs' own, else 'bf16') and `use_graph`, as `HAT` takes them."""

    def __init__(self, naf_width: int = 64, naf_blocks: int = 4, window_size: Optional[int] = None, upscale: int = 2, in_chans: int = 3,
                 hat_kwargs: Optional[dict] = None, compute_dtype: Optional[str] = None, use_graph: bool = False):
        nn.Module.__init__(self)   # (HAT's own constructor builds HAT's tree: this class has another)
        self.naf = _NAFStem(in_ch=in_chans, width=naf_width, n_blocks=naf_blocks)
        # hat_kwargs merged with the top-level keywords: window_size top level > hat_kwargs > 8; upscale / in_chans fill gaps  :109-118
        hk = {} if hat_kwargs is None else dict(hat_kwargs)
        if window_size is None:
            window_size = int(hk.get("window_size", 8))
        hk["window_size"] = int(window_size)
        hk.setdefault("upscale", int(upscale))
        hk.setdefault("in_chans", int(in_chans))
        self.hat = HATX(**hk)
        self.window_size = int(window_size)
        self.upscale = int(hk["upscale"])
        self.in_chans = int(hk["in_chans"])
        self.img_range = getattr(self.hat, "img_range", 1.0)
        self.naf_width, self.naf_blocks = int(naf_width), int(naf_blocks)
        self.cfg = dict(self.hat.cfg, naf=dict(width=self.naf_width, blocks=self.naf_blocks))
        self.compute_dtype = compute_dtype or hk.get("compute_dtype", "bf16")
        self._init_runtime(bool(use_graph))

    def extra_repr(self) -> str:
        return f"window_size={self.window_size}, upscale={self.upscale}, in_chans={self.in_chans}"

    def _anchor(self) -> torch.Tensor:
        return self.naf.head.weight

    def _engine_args(self):
        """The engine reads HATX's parameters by their own names and the stem's under "naf."."""
        return self.cfg, {(k[4:] if k.startswith("hat.") else k): v for k, v in self.state_dict().items()}

    _BANDS = ("a HybridHATNAF frame cannot be sharded into row bands yet: the stem's SCA pool would need one more reduce exchange and "
              "two more halo rows per NAF block (tile_parallel works: it goes through forward)")

    def forward_bands(self, x, n_bands: int):
        raise NotImplementedError(self._BANDS)

    def forward_band_parallel(self, x, group=None):
        raise NotImplementedError(self._BANDS)
