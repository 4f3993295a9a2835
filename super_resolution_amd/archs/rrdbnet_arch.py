"""`RRDBNet` — drop-in for the reference's `basicsr.archs.rrdbnet_arch.RRDBNet` (ESC/basicsr/archs/rrdbnet_arch.py:66-119): the generator
of ESRGAN and of the Real-ESRGAN image models.  Same constructor, same `state_dict()` surface key for key.  Like `HAT`, the module
tree only holds parameters: the forward hands them to `RRDBEngine` (rrdb_engine.py), which runs the network on the MI355X.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .esc_arch import _FixedScaleNet


class ResidualDenseBlock(nn.Module):
    """Five 3x3 convs over the growing concatenation (rrdbnet_arch.py:9-39); parameters only."""

    def __init__(self, num_feat: int = 64, num_grow_ch: int = 32):
        super().__init__()
        for k in range(1, 6):
            setattr(self, f"conv{k}", nn.Conv2d(num_feat + (k - 1) * num_grow_ch, num_grow_ch if k < 5 else num_feat, 3, 1, 1))


class RRDB(nn.Module):
    """Three residual dense blocks (rrdbnet_arch.py:42-63); parameters only."""

    def __init__(self, num_feat: int, num_grow_ch: int = 32):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = (ResidualDenseBlock(num_feat, num_grow_ch) for _ in range(3))


@ARCH_REGISTRY.register()
class RRDBNet(_FixedScaleNet):
    """conv_first, num_block x RRDB (each three residual dense blocks of five convs, every residual scaled by 0.2), conv_body plus
    conv_first's map, two nearest x2 steps with a conv and LeakyReLU 0.2 each, conv_hr, conv_last.  At scale 2 / 1 the frame is
    pixel-unshuffled by 2 / 4 first, so the body runs at half / quarter size and the x4 head gives x2 / x1.  It is a `HAT` from the
    engine up — `compute_dtype` / `set_compute_dtype`, `use_graph` and the weight-change tracking are HAT's own — and a network of the
    ESC family at the frame boundary: `upscale_u8`, `upscale_gt_u8`, `upscale_to_u8`, `upscale_yuv`, `upscale_ensemble`, on batches.

    Built: num_feat 64, num_grow_ch 32, num_in_ch = num_out_ch = 3, scale 1, 2 or 4, any num_block >= 0; anything else is a ValueError
    when the engine packs.  That includes scale 3 and 8, which the reference's constructor accepts and its forward silently treats
    as 4 (rrdbnet_arch.py:106-111): a x3 option file would get a x4 image, so it is refused here.  `forward` refuses a frame that the
    unshuffle factor does not divide with the reference's AssertionError (arch_util.py:198); the frame calls reflect-pad to it and
    crop.  Extra (non-reference) keywords: `compute_dtype` ('bf16' | 'fp32') and `use_graph`."""
    _NAME = "RRDBNet"   # in the refusals _FixedScaleNet words (forward, the byte paths, HAT's forward_* names, row bands)

    def __init__(self, num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32, compute_dtype: str = "bf16", use_graph: bool = False):
        nn.Module.__init__(self)   # (HAT's own constructor builds HAT's tree: this class has another)
        self.scale = self.upscale = scale
        self.cfg = dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, scale=scale, num_feat=num_feat, num_block=num_block, num_grow_ch=num_grow_ch)
        cin = num_in_ch * (4 if scale == 2 else 16 if scale == 1 else 1)
        self.conv_first = nn.Conv2d(cin, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch=num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self.in_chans, self.img_range = num_in_ch, 1.0
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    def _anchor(self) -> torch.Tensor:
        return self.conv_first.weight

    def load_state_dict(self, state_dict, strict=True, assign=False):   # (no `to_img` conversion: the keys are the reference's own)
        return nn.Module.load_state_dict(self, state_dict, strict, assign)

    def _make_engine(self, device):
        from ..rrdb_engine import RRDBEngine
        return RRDBEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
