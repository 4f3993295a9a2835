"""`ESCReal` — drop-in for the reference's `hat.archs.esc_real_arch.ESCReal` (esc_real_arch.py:402-475; the same file ships as
ESC/esc/archs/esc_real_arch.py): the real-world x4 network of the ESC family, same constructor, same `state_dict()` surface key for
key.  The body is `ESC` with LayerNorms in front of every conv block (`lns.*` are always present); on top of it come the `skip`
branch on the input image (1x1, depthwise 7x7 with reflect padding, LeakyReLU 0.2, 1x1) and one of two `to_img` heads: "nearest +
conv" (default) or DySample (`use_dysample=True`, esc_real_arch.py:312-399).  The module tree only holds parameters;
`ESCRealEngine` (esc_engine.py) runs them on the MI355X.

Two behaviours of the reference are kept as they are:
  * the default head is two hard-coded nearest x2 steps: it produces a x4 image whatever `upscaling_factor` says
    (upscaling_factor=2 on 33x40 gives 132x160);
  * the DySample head honours `upscaling_factor` (2, 3 and 4 are built); `to_img.init_pos` has 2 * 4 * s^2 entries.
The reference has no `convert()` and no `to_img` scale conversion in `load_state_dict` for this network; neither has this class.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .esc_arch import ESC, _Block
from .hat_arch import HAT, _Holder


class _DySample(_Holder):  # esc_real_arch.py:312-359
    def __init__(self, in_channels, out_ch, scale, groups=4):
        super().__init__()
        out_channels = 2 * groups * scale ** 2
        self.scale, self.groups = scale, groups
        self.end_conv = nn.Conv2d(in_channels, out_ch, kernel_size=1)
        self.offset = nn.Conv2d(in_channels, out_channels, 1)
        self.scope = nn.Conv2d(in_channels, out_channels, 1, bias=False)
        nn.init.trunc_normal_(self.offset.weight, std=0.02)
        nn.init.constant_(self.scope.weight, val=0)
        self.register_buffer("init_pos", self._init_pos())

    def _init_pos(self) -> torch.Tensor:  # esc_real_arch.py:352-359
        h = torch.arange((-self.scale + 1) / 2, (self.scale - 1) / 2 + 1) / self.scale
        return torch.stack(torch.meshgrid([h, h], indexing="ij")).transpose(1, 2).repeat(1, self.groups, 1).reshape(1, -1, 1, 1)


_NOT_BUILT = "ESCReal has no {}: the reference (esc_real_arch.py:402-475) has none"


@ARCH_REGISTRY.register()
class ESCReal(ESC):
    """ESCReal on the MI355X.  Everything from the engine up is `ESC`'s (and through it `HAT`'s): `compute_dtype`, `use_graph`, the
    weight-change tracking, `tile_parallel`, the `ESRModel` harness.

    Built: ESC's limits (dim 64, pdim 16, kernel_size 13, window_size 32, num_heads 4, exp_ratio 1.25 or 2, any n_blocks /
    conv_blocks), checked when the engine packs; one frame per forward; frames with a side below 4 are refused (the skip branch's
    reflect pad of 3).  The default head outputs x4 whatever `upscaling_factor`; DySample outputs x`upscaling_factor` (2, 3, 4).
    Frames go in and out under the `upscale_*` names (`upscale_u8`, `upscale_gt_u8`, `upscale_to_u8`, `upscale_yuv`, `upscale_ensemble`: DESIGN.md §4.21);
    HAT's `forward_ensemble` / `forward_u8` / `forward_yuv` names, row bands and plans raise NotImplementedError, as for `ESC`."""

    def __init__(self, dim: int, pdim: int, kernel_size: int, n_blocks: int, conv_blocks: int, window_size: int, num_heads: int,
                 upscaling_factor: int, exp_ratio: int = 2, attn_type: str = 'Flex', use_dysample: bool = False,
                 compute_dtype: str = "bf16", use_graph: bool = False):
        nn.Module.__init__(self)
        if attn_type not in ('Naive', 'SDPA', 'Flex'):
            raise NotImplementedError(f'Attention type {attn_type} is not supported.')
        self.plk_filter = nn.Parameter(torch.randn(pdim, pdim, kernel_size, kernel_size))
        torch.nn.init.orthogonal_(self.plk_filter)
        self.proj = nn.Conv2d(3, dim, 3, 1, 1)
        self.blocks = nn.ModuleList([_Block(dim, pdim, conv_blocks, window_size, num_heads, exp_ratio, True) for _ in range(n_blocks)])
        self.last = nn.Conv2d(dim, dim, 3, 1, 1)
        if use_dysample:
            self.to_img = _DySample(dim, 3, upscaling_factor, groups=4)
        else:   # two nearest x2 steps, whatever upscaling_factor says (esc_real_arch.py:447-458)
            self.to_img = nn.Sequential(
                nn.UpsamplingNearest2d(scale_factor=2), nn.Conv2d(dim, dim, 3, 1, 1), nn.LeakyReLU(0.2, inplace=True),
                nn.UpsamplingNearest2d(scale_factor=2), nn.Conv2d(dim, dim, 3, 1, 1), nn.LeakyReLU(0.2, inplace=True),
                nn.Conv2d(dim, dim, 3, 1, 1), nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(dim, 3, 3, 1, 1))
        self.upscaling_factor = int(upscaling_factor)
        self.upscale = int(upscaling_factor) if use_dysample else 4   # what the forward produces: the harness and tile_parallel size by it
        self.skip = nn.Sequential(nn.Conv2d(3, dim * 2, 1, 1, 0), nn.Conv2d(dim * 2, dim * 2, 7, 1, 3, groups=dim * 2, padding_mode='reflect'),
                                  nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(dim * 2, dim, 1, 1, 0))
        self.window_size, self.attn_type, self.in_chans, self.img_range = int(window_size), attn_type, 3, 1.0
        self.use_dysample = bool(use_dysample)
        self.cfg = dict(dim=dim, pdim=pdim, kernel_size=kernel_size, n_blocks=n_blocks, conv_blocks=conv_blocks, window_size=window_size,
                        num_heads=num_heads, upscaling_factor=int(upscaling_factor), exp_ratio=exp_ratio, use_ln=True, converted=False,
                        use_dysample=bool(use_dysample))
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    @property
    def convert(self):
        raise AttributeError(_NOT_BUILT.format("convert()"))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Plain loading: no `to_img` scale conversion (ESC's is for its sub-pixel conv; this network's heads have none)."""
        return HAT.load_state_dict(self, state_dict, strict, assign)

    def _make_engine(self, device):
        from ..esc_engine import ESCRealEngine
        return ESCRealEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
