"""`ESCRealM` — drop-in for the reference's `hat.archs.esc_real_arch.ESCRealM` (esc_real_arch.py:478-661): "ESC-Real for multiple
upscaling factors", same constructor, same `state_dict()` surface key for key.  The body is ESCReal's (the reference's `Block`,
esc_real_arch.py:267-295, always carries its per-conv-block LayerNorms `lns.*`).  Around it:
  * the unshuffled stem: with `unshuffle_mod` and `upscaling_factor < 3` a `PixelUnshuffle(4 // s)` sits in front of `proj` and
    `skip` (keys `proj.1.*`, `skip.1.* / 2.* / 4.*`), the frame is reflect-padded to a multiple of it, the body runs at 1/2 or 1/4
    of the frame size, the head is x4 and the output is cropped to (s h, s w);
  * `to_img` is a `UniUpsample` (esc_real_arch.py:478-574): "conv", "pixelshuffledirect", "pixelshuffle", "nearest+conv" or
    "dysample", with the `MetaUpsample` uint8 buffer in the `state_dict`.
The module tree only holds parameters; `ESCRealMEngine` (esc_engine.py) runs them on the MI355X.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..packing import UNI_UPSAMPLERS
from ..registry import ARCH_REGISTRY
from .esc_arch import _Block, _FixedScaleNet
from .esc_real_arch import _DySample
from .hat_arch import HAT


class _UniUpsample(nn.Sequential):  # esc_real_arch.py:478-574
    def __init__(self, upsample, scale=2, in_dim=64, out_dim=3, mid_dim=64, group=4):
        m = []
        pow2 = (scale & (scale - 1)) == 0
        bad_scale = f"scale {scale} is not supported. Supported scales: 2^n and 3."
        if scale == 1 or upsample == "conv":
            m.append(nn.Conv2d(in_dim, out_dim, 3, 1, 1))
        elif upsample == "pixelshuffledirect":
            m.extend([nn.Conv2d(in_dim, out_dim * scale ** 2, 3, 1, 1), nn.PixelShuffle(scale)])
        elif upsample == "pixelshuffle":
            m.extend([nn.Conv2d(in_dim, mid_dim, 3, 1, 1), nn.LeakyReLU(inplace=True)])
            if pow2:
                for _ in range(int(math.log2(scale))):
                    m.extend([nn.Conv2d(mid_dim, 4 * mid_dim, 3, 1, 1), nn.PixelShuffle(2)])
            elif scale == 3:
                m.extend([nn.Conv2d(mid_dim, 9 * mid_dim, 3, 1, 1), nn.PixelShuffle(3)])
            else:
                raise ValueError(bad_scale)
            m.append(nn.Conv2d(mid_dim, out_dim, 3, 1, 1))
        elif upsample == "nearest+conv":
            if pow2:
                for _ in range(int(math.log2(scale))):
                    m.extend((nn.Conv2d(in_dim, in_dim, 3, 1, 1), nn.Upsample(scale_factor=2), nn.LeakyReLU(negative_slope=0.2, inplace=True)))
                m.extend((nn.Conv2d(in_dim, in_dim, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True)))
            elif scale == 3:
                m.extend((nn.Conv2d(in_dim, in_dim, 3, 1, 1), nn.Upsample(scale_factor=scale), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                          nn.Conv2d(in_dim, in_dim, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True)))
            else:
                raise ValueError(bad_scale)
            m.append(nn.Conv2d(in_dim, out_dim, 3, 1, 1))
        elif upsample == "dysample":
            if mid_dim != in_dim:
                m.extend([nn.Conv2d(in_dim, mid_dim, 3, 1, 1), nn.LeakyReLU(inplace=True)])
            m.append(_DySample(mid_dim, out_dim, scale, group))
        else:
            raise ValueError("An invalid Upsample was selected. Please choose one of typing.Literal['conv', 'pixelshuffledirect', "
                             "'pixelshuffle', 'nearest+conv', 'dysample']")
        super().__init__(*m)
        self.register_buffer("MetaUpsample", torch.tensor([2, UNI_UPSAMPLERS.index(upsample), scale, in_dim, out_dim, mid_dim, group],
                                                          dtype=torch.uint8))


@ARCH_REGISTRY.register()
class ESCRealM(_FixedScaleNet):
    """ESCRealM on the MI355X.  Everything from the engine up is the ESC family's (and through it `HAT`'s): `compute_dtype`,
    `use_graph`, the weight-change tracking, `tile_parallel`, the `ESRModel` harness.

    Built: ESC's limits (dim 64, pdim 16, kernel_size 13, window_size 32, num_heads 4, exp_ratio 1.25 or 2, any n_blocks /
    conv_blocks); upscaling_factor 1..4; `mid_dim` a multiple of 16 for "pixelshuffle", 48 or 64 for "dysample"; "conv" only on the
    plain stem; all checked when the engine packs.  One frame per forward; the body's frame needs sides of at least 4.
    Frames go in and out under the `upscale_*` names (`upscale_u8`, `upscale_gt_u8`, `upscale_to_u8`, `upscale_yuv`, `upscale_ensemble`: DESIGN.md §4.21);
    HAT's `forward_ensemble` / `forward_u8` / `forward_yuv` names, row bands and plans raise NotImplementedError, as for `ESC`."""

    def __init__(self, dim: int, pdim: int, kernel_size: int, n_blocks: int, conv_blocks: int, window_size: int, num_heads: int,
                 upscaling_factor: int, exp_ratio: int = 2, attn_type: str = 'Flex', mid_dim: int = 48, upsampler: str = "nearest+conv",
                 unshuffle_mod: bool = True, compute_dtype: str = "bf16", use_graph: bool = False):
        nn.Module.__init__(self)
        self.upscaling_factor = int(upscaling_factor)
        if attn_type not in ('Naive', 'SDPA', 'Flex'):
            raise NotImplementedError(f'Attention type {attn_type} is not supported.')
        self.plk_filter = nn.Parameter(torch.randn(pdim, pdim, kernel_size, kernel_size))
        torch.nn.init.orthogonal_(self.plk_filter)
        unshuffle, scale = 0, int(upscaling_factor)
        if unshuffle_mod and upscaling_factor < 3:
            unshuffle, scale = 4 // upscaling_factor, 4
            self.proj = nn.Sequential(nn.PixelUnshuffle(unshuffle), nn.Conv2d(3 * unshuffle ** 2, dim, 3, 1, 1))
            self.skip = nn.Sequential(nn.PixelUnshuffle(unshuffle), nn.Conv2d(3 * unshuffle ** 2, dim * 2, 1, 1, 0),
                                      nn.Conv2d(dim * 2, dim * 2, 7, 1, 3, groups=dim * 2, padding_mode='reflect'),
                                      nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(dim * 2, dim, 1, 1, 0))
        else:
            self.proj = nn.Conv2d(3, dim, 3, 1, 1)
            self.skip = nn.Sequential(nn.Conv2d(3, dim * 2, 1, 1, 0), nn.Conv2d(dim * 2, dim * 2, 7, 1, 3, groups=dim * 2, padding_mode='reflect'),
                                      nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(dim * 2, dim, 1, 1, 0))
        self.padding = unshuffle
        self.blocks = nn.ModuleList([_Block(dim, pdim, conv_blocks, window_size, num_heads, exp_ratio, True) for _ in range(n_blocks)])
        self.last = nn.Conv2d(dim, dim, 3, 1, 1)
        self.to_img = _UniUpsample(upsampler, scale, dim, 3, mid_dim, 4)
        # what the forward produces: the harness and tile_parallel size by it ("conv" has no upsampling step at all)
        self.upscale = 1 if (upsampler == "conv" or scale == 1) else int(upscaling_factor)
        self.window_size, self.attn_type, self.in_chans, self.img_range = int(window_size), attn_type, 3, 1.0
        self.cfg = dict(dim=dim, pdim=pdim, kernel_size=kernel_size, n_blocks=n_blocks, conv_blocks=conv_blocks, window_size=window_size,
                        num_heads=num_heads, upscaling_factor=int(upscaling_factor), exp_ratio=exp_ratio, use_ln=True, converted=False,
                        mid_dim=int(mid_dim), upsampler=upsampler, unshuffle=unshuffle, head_scale=scale)
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    def _anchor(self) -> torch.Tensor:
        return self.last.weight

    @property
    def convert(self):
        raise AttributeError("ESCRealM has no convert(): the reference (esc_real_arch.py:578-661) has none")

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """esc_real_arch.py:641-643: the checkpoint's `to_img.MetaUpsample` is replaced by the module's own; no `to_img` scale
        conversion (that is ESC's, for its sub-pixel conv)."""
        state_dict = dict(state_dict)
        state_dict["to_img.MetaUpsample"] = self.to_img.MetaUpsample
        return HAT.load_state_dict(self, state_dict, strict, assign)

    def _make_engine(self, device):
        from ..esc_engine import ESCRealMEngine
        return ESCRealMEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
