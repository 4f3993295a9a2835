"""`ESCFP` — drop-in for the reference's `hat.archs.esc_fp_arch.ESCFP` (esc_fp_arch.py:277-355; the same file ships as
ESC/esc/archs/esc_fp_arch.py): the small network of the ESC family (ESC_FP_X2 / X3 / X4: 48 channels, 3 heads), same constructor,
same `state_dict()` surface key for key, the `to_img` conversion of `load_state_dict`.  Against `ESC`:

  * `Block.proj` is ConvFFN(dim, 3, 1.5); every conv block has its LayerNorm (`lns.*` always present); `ln_last` precedes `last`;
  * the large-kernel branch is DECOMPOSED: `lk_channel` (pdim, pdim, 1, 1; a 1x1 conv without bias) then a depthwise 13x13 whose
    kernel is `lk_spatial` (pdim, 1, 13, 13) plus the instance's dynamic 3x3 (`plk.proj`: pool -> pdim/4 -> GELU -> 9 pdim) on its
    centre.  No geometric ensemble and no `convert()`;
  * the base image added to the pixel shuffle is the bicubic upsample of the input, not its nearest repeat;
  * batches are taken: every sample has its own dynamic kernel.

The module tree only holds parameters; `ESCFPEngine` (esc_engine.py) runs them on the MI355X.  DESIGN.md §4.16.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .esc_arch import _ConvFFN, _FixedScaleNet, _LayerNorm, _WindowAttention
from .hat_arch import _Holder


class _DecomposedConvolutionalAttention(_Holder):  # esc_fp_arch.py:89-100
    def __init__(self, pdim):
        super().__init__()
        self.proj = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(pdim, pdim // 4, 1, 1, 0), nn.GELU(), nn.Conv2d(pdim // 4, pdim * 9, 1, 1, 0))


class _DecomposedWrapper(_Holder):  # esc_fp_arch.py:126-131
    def __init__(self, dim, pdim):
        super().__init__()
        self.plk = _DecomposedConvolutionalAttention(pdim)
        self.aggr = nn.Conv2d(dim, dim, 1, 1, 0)


class _Block(_Holder):  # esc_fp_arch.py:247-264
    def __init__(self, dim, pdim, conv_blocks, window_size, num_heads, exp_ratio):
        super().__init__()
        self.ln_proj = _LayerNorm(dim)
        self.proj = _ConvFFN(dim, 3, 1.5)
        self.ln_attn = _LayerNorm(dim)
        self.attn = _WindowAttention(dim, window_size, num_heads)
        self.lns = nn.ModuleList([_LayerNorm(dim) for _ in range(conv_blocks)])
        self.pconvs = nn.ModuleList([_DecomposedWrapper(dim, pdim) for _ in range(conv_blocks)])
        self.convffns = nn.ModuleList([_ConvFFN(dim, 3, exp_ratio) for _ in range(conv_blocks)])
        self.ln_out = _LayerNorm(dim)
        self.conv_out = nn.Conv2d(dim, dim, 3, 1, 1)


@ARCH_REGISTRY.register()
class ESCFP(_FixedScaleNet):
    """ESCFP on the MI355X.  Everything from the engine up is shared with `ESC` (and through it `HAT`'s): `compute_dtype`,
    `use_graph`, the weight-change tracking, `tile_parallel`, the `ESRModel` harness.

    Built: dim 48, pdim 16, kernel_size 13, window_size 32, num_heads 3, int(48 exp_ratio) in {60, 72, 96} (exp_ratio 1.25, 1.5, 2),
    upscaling_factor 2, 3 or 4, any n_blocks / conv_blocks; anything else is a ValueError when the engine packs.  Any batch size.
    `attn_type` selects an implementation in the reference, not a function: all three values run hat_window_attention_r.
    Frames go in and out under the `upscale_*` names (`upscale_u8`, `upscale_gt_u8`, `upscale_to_u8`, `upscale_yuv`, `upscale_ensemble`: DESIGN.md §4.21);
    HAT's `forward_ensemble` / `forward_u8` / `forward_yuv` names, row bands and plans raise NotImplementedError, as for `ESC`.
    Extra (non-reference) keywords: `compute_dtype` ('bf16' | 'fp32') and `use_graph`."""

    def __init__(self, dim: int, pdim: int, kernel_size: int, n_blocks: int, conv_blocks: int, window_size: int, num_heads: int,
                 upscaling_factor: int, exp_ratio: int = 2, attn_type: str = 'Flex', compute_dtype: str = "bf16", use_graph: bool = False):
        nn.Module.__init__(self)   # (HAT's own constructor builds HAT's tree: this class has another)
        if attn_type not in ('Naive', 'SDPA', 'Flex'):
            raise NotImplementedError(f'Attention type {attn_type} is not supported.')
        self.lk_channel = nn.Parameter(torch.randn(pdim, pdim, 1, 1))
        self.lk_spatial = nn.Parameter(torch.randn(pdim, 1, kernel_size, kernel_size))
        torch.nn.init.orthogonal_(self.lk_spatial)
        self.dim = dim
        self.proj = nn.Conv2d(3, dim, 3, 1, 1)
        self.blocks = nn.ModuleList([_Block(dim, pdim, conv_blocks, window_size, num_heads, exp_ratio) for _ in range(n_blocks)])
        self.ln_last = _LayerNorm(dim)
        self.last = nn.Conv2d(dim, dim, 3, 1, 1)
        self.to_img = nn.Conv2d(dim, 3 * upscaling_factor ** 2, 3, 1, 1)
        self.upscaling_factor = self.upscale = int(upscaling_factor)
        self.window_size, self.attn_type, self.in_chans, self.img_range = int(window_size), attn_type, 3, 1.0
        self.cfg = dict(dim=dim, pdim=pdim, kernel_size=kernel_size, n_blocks=n_blocks, conv_blocks=conv_blocks, window_size=window_size,
                        num_heads=num_heads, upscaling_factor=int(upscaling_factor), exp_ratio=exp_ratio, use_ln=True)
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    def _make_engine(self, device):
        from ..esc_engine import ESCFPEngine
        return ESCFPEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
