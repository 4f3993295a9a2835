"""`SRVGGNetCompact` — drop-in for the reference's `hat.archs.srvgg_arch.SRVGGNetCompact` (srvgg_arch.py:6-69; the same file ships as
ESC/basicsr/archs/srvgg_arch.py): the compact VGG-style generator of the Real-ESRGAN video models.  Same constructor, same
`state_dict()` surface key for key.  Like `HAT`, the module tree only holds parameters: the forward hands them to `SRVGGEngine`
(srvgg_engine.py), which runs the network on the MI355X.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .esc_arch import _FixedScaleNet


@ARCH_REGISTRY.register()
class SRVGGNetCompact(_FixedScaleNet):
    """conv 3 -> 64, num_conv x (conv 64 -> 64), each followed by the activation, conv 64 -> 3 s^2, PixelShuffle(s), plus the
    nearest-upsampled input; all arithmetic at the input's size.  It is a `HAT` from the engine up — `compute_dtype` /
    `set_compute_dtype`, `use_graph` and the weight-change tracking are HAT's own — and a network of the ESC family at the frame
    boundary: `upscale_u8`, `upscale_gt_u8`, `upscale_to_u8`, `upscale_yuv`, `upscale_ensemble`, on frames of any size >= 1x1 and on
    batches.

    Built: num_feat 64, num_in_ch = num_out_ch = 3, upscale 1..4, any num_conv >= 0, act_type 'relu', 'prelu' or 'leakyrelu'
    (slope 0.1); anything else is a ValueError when the engine packs.  An unknown act_type is a ValueError here, at construction,
    where the reference fails with UnboundLocalError (srvgg_arch.py:41: `activation` is never bound).  Extra (non-reference)
    keywords: `compute_dtype` ('bf16' | 'fp32') and `use_graph`."""
    _NAME = "SRVGGNetCompact"   # in the refusals _FixedScaleNet words (forward, the byte paths, HAT's forward_* names, row bands)

    def __init__(self, num_in_ch: int = 3, num_out_ch: int = 3, num_feat: int = 64, num_conv: int = 16, upscale: int = 4, act_type: str = 'prelu',
                 compute_dtype: str = "bf16", use_graph: bool = False):
        nn.Module.__init__(self)   # (HAT's own constructor builds HAT's tree: this class has another)
        if act_type not in ('relu', 'prelu', 'leakyrelu'):
            raise ValueError(f"act_type {act_type!r}: expected 'relu', 'prelu' or 'leakyrelu'")
        self.num_in_ch, self.num_out_ch, self.num_feat, self.num_conv, self.upscale, self.act_type = num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type

        def activation():
            if act_type == 'relu':
                return nn.ReLU(inplace=True)
            if act_type == 'prelu':
                return nn.PReLU(num_parameters=num_feat)
            return nn.LeakyReLU(negative_slope=0.1, inplace=True)

        self.body = nn.ModuleList([nn.Conv2d(num_in_ch, num_feat, 3, 1, 1), activation()])
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(num_feat, num_feat, 3, 1, 1))
            self.body.append(activation())
        self.body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(upscale)
        self.in_chans, self.img_range = num_in_ch, 1.0
        self.cfg = dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, num_feat=num_feat, num_conv=num_conv, upscale=upscale, act_type=act_type)
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    def _anchor(self) -> torch.Tensor:
        return self.body[0].weight

    def load_state_dict(self, state_dict, strict=True, assign=False):   # (no `to_img` conversion: the keys are the reference's own)
        return nn.Module.load_state_dict(self, state_dict, strict, assign)

    def _make_engine(self, device):
        from ..srvgg_engine import SRVGGEngine
        return SRVGGEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
