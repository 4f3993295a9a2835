"""`ESC` — drop-in for the reference's `hat.archs.esc_arch.ESC` (esc_arch.py:301-386; the same file ships as
ESC/esc/archs/esc_arch.py): same constructor, same `state_dict()` surface key for key, `convert()` and the `to_img`
conversion of `load_state_dict`.  Like `HAT`, the module tree only holds parameters: the forward hands them to `ESCEngine`
(esc_engine.py), which runs the network on the MI355X.  `attn_type` selects an implementation in the reference, not a function:
all three values run hat_window_attention_r.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..packing import esc_geo_ensemble
from ..registry import ARCH_REGISTRY
from .hat_arch import HAT, _Holder


class _LayerNorm(_Holder):  # esc_arch.py:68-77
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _ConvolutionalAttention(_Holder):  # esc_arch.py:89-102
    def __init__(self, pdim):
        super().__init__()
        self.dwc_proj = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(pdim, pdim // 2, 1, 1, 0), nn.GELU(),
                                      nn.Conv2d(pdim // 2, pdim * 9, 1, 1, 0))
        nn.init.zeros_(self.dwc_proj[-1].weight)
        nn.init.zeros_(self.dwc_proj[-1].bias)


class _ConvAttnWrapper(_Holder):  # esc_arch.py:136-140
    def __init__(self, dim, pdim):
        super().__init__()
        self.plk = _ConvolutionalAttention(pdim)
        self.aggr = nn.Conv2d(dim, dim, 1, 1, 0)


class _ConvFFN(_Holder):  # esc_arch.py:148-153
    def __init__(self, dim, kernel_size, exp_ratio):
        super().__init__()
        hid = int(dim * exp_ratio)
        self.proj = nn.Conv2d(dim, hid, 1, 1, 0)
        self.dwc = nn.Conv2d(hid, hid, kernel_size, 1, kernel_size // 2, groups=hid)
        self.aggr = nn.Conv2d(hid, dim, 1, 1, 0)


class _WindowAttention(_Holder):  # esc_arch.py:162-184
    def __init__(self, dim, window_size, num_heads):
        super().__init__()
        self.to_qkv = nn.Conv2d(dim, dim * 3, 1, 1, 0)
        self.to_out = nn.Conv2d(dim, dim, 1, 1, 0)
        self.relative_position_bias = nn.Parameter(torch.randn(num_heads, (2 * window_size - 1) ** 2).to(torch.float32) * 0.001)


class _Block(_Holder):  # esc_arch.py:256-274
    def __init__(self, dim, pdim, conv_blocks, window_size, num_heads, exp_ratio, use_ln):
        super().__init__()
        self.ln_proj = _LayerNorm(dim)
        self.proj = _ConvFFN(dim, 3, 2)
        self.ln_attn = _LayerNorm(dim)
        self.attn = _WindowAttention(dim, window_size, num_heads)
        self.lns = nn.ModuleList([_LayerNorm(dim) if use_ln else nn.Identity() for _ in range(conv_blocks)])
        self.pconvs = nn.ModuleList([_ConvAttnWrapper(dim, pdim) for _ in range(conv_blocks)])
        self.convffns = nn.ModuleList([_ConvFFN(dim, 3, exp_ratio) for _ in range(conv_blocks)])
        self.ln_out = _LayerNorm(dim)
        self.conv_out = nn.Conv2d(dim, dim, 3, 1, 1)


# {0}: the network's name in messages (_ESCNet._NAME)
_NOT_BUILT = ("{0} runs its float forward only: {1} is not built for it (DESIGN.md §7); `forward` and, through it, "
              "tile_parallel work")
_NEW_NAME = ("{0} runs its float forward only under HAT's forward_* names: {1} is `{2}` in this family (upscale_u8, upscale_gt_u8, "
             "upscale_to_u8, upscale_yuv, upscale_ensemble; DESIGN.md §4.21)")


class _ESCNet(HAT):
    """What the networks of the ESC family share above their module trees: a `HAT` from the engine up — `compute_dtype` /
    `set_compute_dtype`, `use_graph` and the weight-change tracking are HAT's own — with the float forward as the only path, and the
    `to_img` scale conversion of `load_state_dict`.  A subclass builds its tree, sets `cfg`, and names its engine in `_make_engine`."""
    arbitrary_scale = False   # True: the network has no fixed scale and its frame paths take size= / scale= (ESCLTE)
    _NAME = "ESC"             # what the refusals call the network (the family says ESC; SRVGGNetCompact names itself)

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={v}" for k, v in self.cfg.items())

    def _anchor(self) -> torch.Tensor:
        return self.proj.weight

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """esc_arch.py:342-375: a checkpoint of another scale has its `to_img` interpolated bilinearly over the sub-pixel grid."""
        k, b = state_dict.get('to_img.weight'), state_dict.get('to_img.bias')
        s_in, s_out = int((k.shape[0] // 3) ** 0.5), self.upscaling_factor
        if s_in != s_out:
            state_dict = dict(state_dict)
            _, cin, kh, kw = k.shape
            kk = k.reshape(3, s_in, s_in, cin * kh * kw).permute(3, 0, 1, 2)                       # (cin kh kw) rgb rh rw
            kk = F.interpolate(kk, size=(s_out, s_out), mode='bilinear', align_corners=False)
            state_dict['to_img.weight'] = kk.permute(1, 2, 3, 0).reshape(3 * s_out * s_out, cin, kh, kw)
            bb = F.interpolate(b.reshape(1, 3, s_in, s_in), size=(s_out, s_out), mode='bilinear', align_corners=False)
            state_dict['to_img.bias'] = bb.reshape(-1)
        return super().load_state_dict(state_dict, strict, assign)

    def engine(self, device=None):
        """The packed-weight engine for the current parameters (re-packed when they change)."""
        device = torch.device(device) if device is not None else self._anchor().device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = self._weights_key(device) + (self.cfg.get("converted", False),)
        if self._engine is None or self._engine_key != key:
            if self._anchor().device != device:
                raise RuntimeError(f"input is on {device} but the parameters are on {self._anchor().device}: "
                                   f"move the module first (net.to('{device}'))")
            self._engine = self._make_engine(device)
            self._engine_key = key
        return self._engine

    def forward(self, x):
        if self.training:
            raise RuntimeError(f"this {self._NAME} implements the inference forward pass only: call .eval() first (training is out of scope)")
        if not x.is_cuda:
            raise RuntimeError(f"{self._NAME}.forward needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")
        with torch.no_grad():
            from .. import ops
            if self.use_graph and not ops.profiling():
                return self._forward_graph(x)
            return self.engine(x.device).forward(x).to(x.dtype, copy=True)

    def forward_ensemble(self, x, n: int = 8):
        raise NotImplementedError(_NOT_BUILT.format(self._NAME, "forward_ensemble"))

    def forward_to_u8(self, *a, **k):
        raise NotImplementedError(_NOT_BUILT.format(self._NAME, "the byte frame path"))

    forward_u8 = forward_gt_u8 = forward_to_u8

    def forward_yuv420(self, *a, **k):
        raise NotImplementedError(_NOT_BUILT.format(self._NAME, "the YCbCr frame path"))

    forward_yuv = forward_yuv420

    def forward_bands(self, x, n_bands: int):
        raise NotImplementedError(_NOT_BUILT.format(self._NAME, "row-band sharding"))

    def forward_band_parallel(self, x, group=None):
        raise NotImplementedError(_NOT_BUILT.format(self._NAME, "row-band sharding"))


class _FixedScaleNet(_ESCNet):
    """The fixed-scale networks of the family (ESC, ESCReal, ESCRealM, ESCFP): frames in, frames out under the `upscale_*` names, as
    ESCLTE has them.  Semantics, errors and `out=` rules are those of HAT's `forward_*` namesakes, whose module-level wrappers (they
    resolve matrices, devices and batch axes) these calls go through; the engine side is frame_boundary.FrameBoundary on ESCEngine.
    A frame of any size is taken as it is, nothing is padded, and the network's own refusals apply (a reflection larger than the
    frame; a side below 4 for the skip branch; a batch where the network takes one frame).  The result is `upscale` times the frame:
    what the network really applies (ESCReal's default head: 4).  All run eagerly also with use_graph=True.  HAT's own names for
    these calls keep raising NotImplementedError, and say which call took their place.  DESIGN.md §4.21."""

    def _check_u8_input(self, t):   # (HAT's, without in_chans: the family's networks are three-channel)
        if self.training:
            raise RuntimeError(f"this {self._NAME} implements the inference forward pass only: call .eval() first (training is out of scope)")
        if not t.is_cuda:
            raise RuntimeError(f"{self._NAME} needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")

    def forward_ensemble(self, x, n: int = 8):
        raise NotImplementedError(_NEW_NAME.format(self._NAME, "the self-ensemble", "upscale_ensemble"))

    def forward_to_u8(self, *a, **k):
        raise NotImplementedError(_NEW_NAME.format(self._NAME, "the byte frame path", "upscale_u8 / upscale_gt_u8 / upscale_to_u8"))

    forward_u8 = forward_gt_u8 = forward_to_u8

    def forward_yuv420(self, *a, **k):
        raise NotImplementedError(_NEW_NAME.format(self._NAME, "the YCbCr frame path", "upscale_yuv"))

    forward_yuv = forward_yuv420

    def upscale_u8(self, frame, *, bgr: bool = False, out=None, ensemble: int = 1):
        """(h,w,3) or (B,h,w,3) uint8 device frames -> (B,S h,S w,3) uint8: HAT.forward_u8's contract.  Equal to hat_u8_to_planes ->
        `forward` -> hat_planes_to_u8; where the head ends in a fused sink (ESCEngine.u8_fused_calls counts them) no fp32 image is
        written."""
        return HAT.forward_u8(self, frame, bgr=bgr, out=out, ensemble=ensemble)

    def upscale_gt_u8(self, gt, *, bgr: bool = False, out=None, ensemble: int = 1):
        """Ground-truth frames in, the super-resolution of their own bicubic low-resolution image out: HAT.forward_gt_u8's contract
        (a result factor of 2, 3 or 4)."""
        return HAT.forward_gt_u8(self, gt, bgr=bgr, out=out, ensemble=ensemble)

    def upscale_to_u8(self, x, *, crop=None, bgr: bool = False, out=None, ensemble: int = 1):
        """`forward(x)` handed over as bytes: (B,3,H,W) float planes in -> (B,h_out,w_out,3) uint8, crop = (h_out, w_out) the top-left
        pixels kept (default: all of (S H, S W)): HAT.forward_to_u8's contract."""
        self._check_u8_input(x)
        with torch.no_grad():
            return self.engine(x.device).forward_to_u8(x, crop=crop, bgr=bgr, out=out, ensemble=ensemble)

    def upscale_yuv(self, frame, *, fmt: str, out_fmt=None, matrix: str = "bt601", full_range: bool = False, depth: int = 8, out_depth=None,
                    msb=None, out_msb=None, siting: str = "center", out_siting=None, out=None, ensemble: int = 1, width=None):
        """YCbCr frames of any layout of yuv.LAYOUTS or yuv.PACKED_FORMATS in, any out: HAT.forward_yuv's contract.  A centre-sited
        output of a shuffle or conv head is stored by the head's fused sink; a co-sited or packed one is converted from planes
        (hat_planes_to_yuv_sited / hat_planes_to_packed422)."""
        return HAT.forward_yuv(self, frame, fmt=fmt, out_fmt=out_fmt, matrix=matrix, full_range=full_range, depth=depth, out_depth=out_depth,
                               msb=msb, out_msb=out_msb, out=out, ensemble=ensemble, siting=siting, out_siting=out_siting, width=width)

    def upscale_ensemble(self, x, n: int = 8):
        """The geometric self-ensemble of `forward`: HAT.forward_ensemble's contract (n in 1, 2, 4, 8; the transposed members run
        the transposed frame)."""
        from .. import ops
        n = ops.ensemble_members(n)
        self._check_u8_input(x)
        with torch.no_grad():
            return self.engine(x.device).forward_ensemble(x, n).to(x.dtype, copy=n == 1)   # (n = 1: the workspace's buffer)


@ARCH_REGISTRY.register()
class ESC(_FixedScaleNet):
    """The ESC network on the MI355X.  It is a `HAT` from the engine up — `compute_dtype` / `set_compute_dtype`, `use_graph` and the
    weight-change tracking are HAT's own — over a module tree and an engine of its own.

    Built: dim 64, pdim 16, kernel_size 13, window_size 32, num_heads 4, exp_ratio 1.25 or 2, any n_blocks / conv_blocks,
    use_ln either way (ESC, ESC-light, ESCReal's body); anything else is a ValueError when the engine packs.  One frame per
    forward, as in the reference's eval path.  Extra (non-reference) keywords: `compute_dtype` ('bf16' | 'fp32') and `use_graph`."""

    def __init__(self, dim: int, pdim: int, kernel_size: int, n_blocks: int, conv_blocks: int, window_size: int, num_heads: int,
                 upscaling_factor: int, exp_ratio: int = 2, attn_type: str = 'Flex', use_ln: bool = False, compute_dtype: str = "bf16",
                 use_graph: bool = False):
        nn.Module.__init__(self)   # (HAT's own constructor builds HAT's tree: this class has another)
        if attn_type not in ('Naive', 'SDPA', 'Flex'):
            raise NotImplementedError(f'Attention type {attn_type} is not supported.')
        self.plk_filter = nn.Parameter(torch.randn(pdim, pdim, kernel_size, kernel_size))
        torch.nn.init.orthogonal_(self.plk_filter)
        self.proj = nn.Conv2d(3, dim, 3, 1, 1)
        self.blocks = nn.ModuleList([_Block(dim, pdim, conv_blocks, window_size, num_heads, exp_ratio, use_ln) for _ in range(n_blocks)])
        self.last = nn.Conv2d(dim, dim, 3, 1, 1)
        self.to_img = nn.Conv2d(dim, 3 * upscaling_factor ** 2, 3, 1, 1)
        self.upscaling_factor = self.upscale = int(upscaling_factor)
        self.window_size, self.attn_type, self.in_chans, self.img_range = int(window_size), attn_type, 3, 1.0
        self.cfg = dict(dim=dim, pdim=pdim, kernel_size=kernel_size, n_blocks=n_blocks, conv_blocks=conv_blocks, window_size=window_size,
                        num_heads=num_heads, upscaling_factor=int(upscaling_factor), exp_ratio=exp_ratio, use_ln=bool(use_ln), converted=False)
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    @torch.no_grad()
    def convert(self):
        """Bake the geometric re-parameterisation into `plk_filter` (esc_arch.py:337-340); the forward then uses it as it is."""
        if not self.cfg["converted"]:
            self.plk_filter = nn.Parameter(esc_geo_ensemble(self.plk_filter.detach()))
            self.cfg["converted"] = True
            self._plist = None
            self.mark_weights_changed()
        return self

    def _make_engine(self, device):
        from ..esc_engine import ESCEngine
        return ESCEngine(self.cfg, self.state_dict(), device, self.compute_dtype)
