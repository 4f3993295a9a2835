"""`HAT` — drop-in for the reference's `hat.archs.hat_arch.HAT` (hat/archs/hat_arch.py:607-859).

Same constructor kwargs (unknown keys swallowed, :644), same `state_dict()` key/shape/dtype
surface (checked in tests against the reference's own surface), same
registration name `'HAT'`, same call contract: `net(x)` with `x: (B,3,H,W)` float in [0,1],
H and W multiples of `window_size`, returns `(B,3,sH,sW)` float32 on the same device.

The module tree below only HOLDS parameters (nn.Linear / nn.Conv2d / nn.LayerNorm are used as
typed containers so initialisation matches the reference, :761-768).  `forward` never runs a
torch op on them: it hands the parameters to `HATEngine`, which packs them for the MI355X
kernels and enqueues hand-written HIP code through the C ABI (include/hat_mi355x.h).  There is
no CPU path: a CPU tensor or a missing libhat_mi355x.so raises.
"""
from __future__ import annotations

import collections
import math
import os

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY


def _index_table_sa(ws: int) -> torch.Tensor:
    """`relative_position_index_SA` (hat_arch.py:770-781): (qh_i-qh_j+ws-1)*(2ws-1) + (qw_i-qw_j+ws-1).
    Dead on this path (no block consumes it) but part of the state-dict contract."""
    i = torch.arange(ws * ws)
    h, w = i // ws, i % ws
    return ((h[:, None] - h[None, :] + ws - 1) * (2 * ws - 1) + (w[:, None] - w[None, :] + ws - 1)).to(torch.int64)


def _index_table_oca(ws: int, overlap_ratio: float) -> torch.Tensor:
    """`relative_position_index_OCA` (hat_arch.py:783-803); keeps the reference's NEGATIVE values
     for strict state-dict compatibility — the kernels use a rotated table instead."""
    wse = ws + int(overlap_ratio * ws)
    qi, ki = torch.arange(ws * ws), torch.arange(wse * wse)
    off = ws - wse + 1
    dh = (ki // wse)[None, :] - (qi // ws)[:, None] + off
    dw = (ki % wse)[None, :] - (qi % ws)[:, None] + off
    return (dh * (ws + wse - 1) + dw).to(torch.int64)


class _Holder(nn.Module):
    """A module that only owns parameters/sub-modules; calling it is an error by design."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the forward pass runs in HIP kernels via HAT.forward")


class _ECA(_Holder):
    def __init__(self, k_size=5):
        super().__init__()
        self.conv = nn.Conv1d(1, 1, kernel_size=k_size, padding=k_size // 2, bias=False)


class _CAB(_Holder):
    def __init__(self, dim, compress_ratio):
        super().__init__()
        mid = dim // compress_ratio
        self.cab = nn.Sequential(nn.Conv2d(dim, mid, 3, 1, 1), nn.GELU(), nn.Conv2d(mid, dim, 3, 1, 1), _ECA(5))


class _ConvAttn(_Holder):  # esc_arch.py:89-102
    def __init__(self, pdim):
        super().__init__()
        self.dwc_proj = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(pdim, pdim // 2, 1, 1, 0), nn.GELU(),
                                      nn.Conv2d(pdim // 2, pdim * 9, 1, 1, 0))
        nn.init.zeros_(self.dwc_proj[-1].weight)
        nn.init.zeros_(self.dwc_proj[-1].bias)


class _ConvAttnWrapper(_Holder):  # esc_arch.py:136-140
    def __init__(self, dim, pdim):
        super().__init__()
        self.plk = _ConvAttn(pdim)
        self.aggr = nn.Conv2d(dim, dim, 1, 1, 0)


class _ESCAttn(_Holder):  # hat_arch.py:139-149
    def __init__(self, dim, pdim, ksize):
        super().__init__()
        self.core = _ConvAttnWrapper(dim, pdim)
        self.plk_filter = nn.Parameter(torch.randn(pdim, pdim, ksize, ksize))
        nn.init.orthogonal_(self.plk_filter)


class _FFN(_Holder):  # hat_arch.py:95-105
    def __init__(self, dim, mlp_ratio):
        super().__init__()
        hidden = int(dim * mlp_ratio)
        self.fc1 = nn.Linear(dim, 2 * hidden)
        self.dw = nn.Conv2d(2 * hidden, 2 * hidden, 3, 1, 1, groups=2 * hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _SGFN(_Holder):  # hatx_arch.py:144-158 (SpatialGateDConvFFN): the depthwise conv covers the first half only
    def __init__(self, dim, mlp_ratio):
        super().__init__()
        hidden = int(dim * mlp_ratio)
        assert hidden % 2 == 0, f"Hidden({hidden}) must be even for spatial gate split."
        self.fc1 = nn.Linear(dim, hidden)
        self.dw = nn.Conv2d(hidden // 2, hidden // 2, 3, 1, 1, groups=hidden // 2)
        self.fc2 = nn.Linear(hidden, dim)


class _HAB(_Holder):  # hat_arch.py:172-215 (sgfn: hatx_arch.py:185-230)
    def __init__(self, dim, compress_ratio, mlp_ratio, esc_pdim, esc_kernel, sgfn=False):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.esc_attn = _ESCAttn(dim, esc_pdim, esc_kernel)
        self.conv_block = _CAB(dim, compress_ratio)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _SGFN(dim, mlp_ratio) if sgfn else _FFN(dim, mlp_ratio)


class _OCAB(_Holder):  # hat_arch.py:267-324
    def __init__(self, dim, window_size, overlap_ratio, num_heads, qkv_bias, mlp_ratio, esc_enable, esc_pdim, esc_kernel,
                 focus=False):
        super().__init__()
        wse = int(window_size * overlap_ratio) + window_size
        self.norm1 = nn.LayerNorm(dim)
        self.q_proj = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv_proj = nn.Linear(dim, 2 * dim, bias=qkv_bias)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((window_size + wse - 1) ** 2, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        hid = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, hid), nn.GELU(), nn.Linear(hid, dim))
        if esc_enable:
            self.esc_core = _ConvAttnWrapper(dim, esc_pdim)
            self.esc_plk = nn.Parameter(torch.randn(esc_pdim, esc_pdim, esc_kernel, esc_kernel))
            nn.init.orthogonal_(self.esc_plk)
        if focus:  # hatx_arch.py:357-361: saliency head of the focus bias
            self.focus_head = nn.Sequential(nn.Conv2d(dim, dim // 4, 1, 1, 0), nn.GELU(), nn.Conv2d(dim // 4, 1, 1, 1, 0))


class _AttenBlocks(_Holder):  # hat_arch.py:395-464
    def __init__(self, dim, depth, num_heads, window_size, compress_ratio, overlap_ratio, mlp_ratio, qkv_bias, esc_pdim,
                 esc_kernel, ocab_esc_enable, ocab_esc_pdim, ocab_esc_kernel, sgfn=False, focus=False):
        super().__init__()
        self.blocks = nn.ModuleList([_HAB(dim, compress_ratio, mlp_ratio, esc_pdim, esc_kernel, sgfn) for _ in range(depth)])
        self.overlap_attn = _OCAB(dim, window_size, overlap_ratio, num_heads, qkv_bias, mlp_ratio, ocab_esc_enable,
                                  ocab_esc_pdim, ocab_esc_kernel, focus)


class _RHAG(_Holder):  # hat_arch.py:484-553
    def __init__(self, dim, resi_connection, **kw):
        super().__init__()
        self.residual_group = _AttenBlocks(dim, **kw)
        if resi_connection == '1conv':
            self.conv = nn.Conv2d(dim, dim, 3, 1, 1)
        elif resi_connection == 'identity':
            self.conv = nn.Identity()
        else:
            raise ValueError(f"Unknown resi_connection: {resi_connection}")


class _PatchEmbed(_Holder):  # hat_arch.py:558-570
    def __init__(self, embed_dim, norm_layer):
        super().__init__()
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None


class _Upsample(nn.Sequential):  # hat_arch.py:593-605
    def __init__(self, scale, num_feat):
        m = []
        if (scale & (scale - 1)) == 0:
            for _ in range(int(math.log(scale, 2))):
                m.append(nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1))
                m.append(nn.PixelShuffle(2))
        elif scale == 3:
            m.append(nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1))
            m.append(nn.PixelShuffle(3))
        else:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        super().__init__(*m)


@ARCH_REGISTRY.register()
class HAT(nn.Module):
    """Hybrid Attention Transformer (this fork: ESC conv-attention HABs + OCAB), MI355X-native forward.

    Extra (non-reference) constructor keyword: `compute_dtype` in {'bf16', 'f32'} selects the
    kernel storage/MFMA type (default 'bf16'; 'f32' is the exact-fp32 parity path).  It can also
    be changed later with `set_compute_dtype`.
    """
    _VARIANT = "hat"

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6),
                 window_size=7, compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.,
                 upsampler='', resi_connection='1conv', esc_pdim: int = 16, esc_kernel: int = 13,
                 esc_use_dynamic: bool = True, ocab_esc_enable: bool = False, ocab_esc_pdim: int = 16,
                 ocab_esc_kernel: int = 13, compute_dtype: str = 'bf16', **kwargs):
        super().__init__()
        self.cfg = dict(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                        depths=tuple(depths), num_heads=tuple(num_heads), window_size=window_size,
                        compress_ratio=compress_ratio, squeeze_factor=squeeze_factor, conv_scale=conv_scale,
                        overlap_ratio=overlap_ratio, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, ape=ape,
                        patch_norm=patch_norm, upscale=upscale, img_range=img_range, upsampler=upsampler,
                        resi_connection=resi_connection, esc_pdim=esc_pdim, esc_kernel=esc_kernel,
                        ocab_esc_enable=ocab_esc_enable, ocab_esc_pdim=ocab_esc_pdim, ocab_esc_kernel=ocab_esc_kernel,
                        variant=self._VARIANT, kv_topk_ratio=float(kwargs.get("_kv_topk_ratio", 1.0)),
                        use_focus_bias=bool(kwargs.get("_use_focus_bias", False)))
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.overlap_ratio = overlap_ratio
        self.img_range = img_range
        self.upscale = upscale
        self.upsampler = upsampler
        self.embed_dim = embed_dim
        self.num_layers = len(depths)
        self.compute_dtype = compute_dtype
        num_feat = 64  # hard-coded in the reference (:656)
        if in_chans == 3:
            self.mean = torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1)
        else:
            self.mean = torch.zeros(1, 1, 1, 1)

        self.register_buffer('relative_position_index_SA', _index_table_sa(window_size))
        self.register_buffer('relative_position_index_OCA', _index_table_oca(window_size, overlap_ratio))

        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, norm_layer if patch_norm else None)
        if ape:
            n = (img_size // patch_size) ** 2
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, n, embed_dim))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=.02)
        self.layers = nn.ModuleList([
            _RHAG(embed_dim, resi_connection, depth=depths[i], num_heads=num_heads[i], window_size=window_size,
                  compress_ratio=compress_ratio, overlap_ratio=overlap_ratio, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                  esc_pdim=esc_pdim, esc_kernel=esc_kernel, ocab_esc_enable=ocab_esc_enable, ocab_esc_pdim=ocab_esc_pdim,
                  ocab_esc_kernel=ocab_esc_kernel, sgfn=self._VARIANT == "hatx",
                  focus=bool(kwargs.get("_use_focus_bias", False))) for i in range(self.num_layers)])
        self.norm = norm_layer(embed_dim)
        if resi_connection == '1conv':
            self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        elif resi_connection == 'identity':
            self.conv_after_body = nn.Identity()
        else:
            raise ValueError(f"Unknown resi_connection: {resi_connection}")
        if self.upsampler == 'pixelshuffle':
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.upsample = _Upsample(upscale, num_feat)
            self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
        self.apply(self._init_weights)
        self._init_runtime(bool(kwargs.get("use_graph", False)))

    def _init_runtime(self, use_graph: bool):
        """What the device forward keeps beside the parameters: the packed engine, the weight-change tracking, the graph cache."""
        self._engine = None
        self._engine_key = None
        self._wver = 0   # bumped whenever the parameters may have changed (load_state_dict, .to()/.cuda()/..., explicit)
        self._plist = None
        self.register_load_state_dict_post_hook(HAT._post_load_hook)
        # extra (non-reference) switch: replay the forward as a HIP graph (also HAT_GRAPH=1 in the environment)
        self.use_graph = use_graph or os.environ.get("HAT_GRAPH") == "1"
        self._graphs, self._graph_engine = collections.OrderedDict(), None
        self._graph_max = int(os.environ.get("HAT_GRAPH_CACHE", "4"))

    def _anchor(self) -> torch.Tensor:
        """The parameter whose device is the module's."""
        return self.conv_first.weight

    def _engine_args(self):
        """(cfg, state dict) the engine packs."""
        return self.cfg, self.state_dict()

    def _init_weights(self, m):  # hat_arch.py:761-768
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'absolute_pos_embed'}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table'}

    # ------------------------------------------------------------------------------------------
    def set_compute_dtype(self, dtype: str):
        self.compute_dtype = dtype
        self._engine = None
        return self

    # The engine holds PACKED copies of the parameters.  It is rebuilt when the weights key changes.  The key is cheap
    # (a walk over data_ptr of ~900 parameters on every forward was ~1.5 ms, a third of a 64x64 forward) and has two parts:
    #   * `_wver`, bumped by every bulk path that rewrites parameters: a load_state_dict POST HOOK (fires for this module
    #     also when the call was made on a parent / wrapper — nn.DataParallel(net), nn.Sequential(net), a user container —
    #     where torch recurses through _load_from_state_dict and never calls the child's load_state_dict), `_apply`
    #     (.to / .cuda / .float / ...) and `mark_weights_changed()`;
    #   * the sum of `p._version` over a cached parameter list (~0.1 ms for HAT-S's 910 parameters): catches every in-place edit autograd sees —
    #     optimizer steps, `p.copy_()`, `p.mul_()` under no_grad.
    # What this cannot see: an edit made through `p.data` (`p.data.mul_(d)`: `.data` has its own version counter by design,
    # e.g. BasicSR's EMA update) and a parameter OBJECT replaced on a submodule (`net.conv_first.weight = nn.Parameter(..)`):
    # such code must call `mark_weights_changed()` (the walk that would find them costs 1.5 ms).  HAT_STRICT_WEIGHTS=1 restores the
    # full per-forward walk over (data_ptr, _version) for debugging.
    def mark_weights_changed(self):
        self._wver += 1
        return self

    @staticmethod
    def _post_load_hook(module, incompatible_keys):
        module._wver = getattr(module, "_wver", 0) + 1

    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self._wver = getattr(self, "_wver", 0) + 1
        self._plist = None
        return r

    def _weights_key(self, device):
        pl = getattr(self, "_plist", None)
        if pl is None or self._plist_wver != self._wver:
            pl = self._plist = list(self.parameters())
            self._plist_wver = self._wver
        key = (str(device), self.compute_dtype, self._wver, sum(p._version for p in pl))
        if os.environ.get("HAT_STRICT_WEIGHTS") == "1":
            key += tuple((p.data_ptr(), p._version) for p in self.parameters())
        return key

    def engine(self, device=None):
        """The packed-weight engine for the current parameters (re-packed when they change)."""
        from ..engine import HATEngine
        device = torch.device(device) if device is not None else self._anchor().device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = self._weights_key(device)
        if self._engine is None or self._engine_key != key:
            if self._anchor().device != device:
                raise RuntimeError(f"input is on {device} but the parameters are on {self._anchor().device}: "
                                   f"move the module first (net.to('{device}'))")
            self._engine = HATEngine(*self._engine_args(), device, self.compute_dtype)
            self._engine_key = key
        return self._engine

    def forward(self, x):
        if self.training:
            raise RuntimeError("this HAT implements the inference forward pass only: call .eval() first "
                               "(training is out of scope, SURVEY §2)")
        if not x.is_cuda:
            raise RuntimeError("HAT.forward needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")
        with torch.no_grad():
            from .. import ops
            if self.use_graph and not ops.profiling():
                return self._forward_graph(x)
            return self.engine(x.device).forward(x).to(x.dtype)

    def forward_ensemble(self, x, n: int = 8):
        """The geometric self-ensemble of `forward` (the "+" of SR evaluation; the reference's SRModel.test_selfensemble, basicsr
        models/sr_model.py:132-178, without its host round trips): the network on the first n of the eight flips / transposes of
        x, every output transformed back, the mean of the n — all on the device (hat_dihedral_f32).  n in {1, 2, 4, 8}
        (ValueError otherwise); member i = v | h << 1 | t << 2 with v: reverse W, h: reverse H, t: swap H and W, applied in that
        order, so n = 4 runs no transposed shape and n = 1 is forward(x) bit for bit.  fp32 accumulation in member order, acc +=
        (1 / n) * T_i^-1(y_i).  Input, output and refusals are forward's.  Runs eagerly also with use_graph=True (the ensemble
        is not captured)."""
        from .. import ops
        n = ops.ensemble_members(n)
        if self.training:
            raise RuntimeError("this HAT implements the inference forward pass only: call .eval() first "
                               "(training is out of scope, SURVEY §2)")
        if not x.is_cuda:
            raise RuntimeError("HAT.forward needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")
        with torch.no_grad():
            return self.engine(x.device).forward_ensemble(x, n).to(x.dtype)

    # ---- the 8-bit frame boundary (no counterpart in the reference's module: its caller converts on the host,
    # basicsr utils/img_util.py:9-35, :66-91, :131 and hat/models/hat_model.py:16-26, :110-112) ----
    def _check_u8_input(self, t):
        if self.training:
            raise RuntimeError("this HAT implements the inference forward pass only: call .eval() first")
        if not t.is_cuda:
            raise RuntimeError("HAT.forward needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")
        if self.cfg["in_chans"] != 3:
            raise RuntimeError(f"8-bit frames are three-channel images: in_chans={self.cfg['in_chans']} has no uint8 path")

    def forward_to_u8(self, x, *, bgr: bool = False, out=None, ensemble: int = 1):
        """`forward(x)` handed over as an 8-bit image: (B,3,H,W) float in [0,1], H and W window multiples as for `forward`
        -> (B,sH,sW,3) uint8 on the device, equal to the reference's `tensor2img` of `forward(x)` (clamp to [0,1], x255 in
        fp32, round half to even, CHW -> HWC; bgr=True: B,G,R byte order).  On the bf16 path conv_last converts in its
        epilogue and the fp32 image is never written.  out: a (B,sH,sW,3) uint8 device tensor to fill instead of a fresh one.
        Runs eagerly also with use_graph=True (the 8-bit path is not captured).
        ensemble 2 / 4 / 8: `forward_ensemble(x, ensemble)` handed over in the same way (hat_planes_to_u8 converts its fp32 image);
        ensemble=1 is the call as it always was."""
        self._check_u8_input(x)
        with torch.no_grad():
            return self.engine(x.device).forward_to_u8(x, bgr=bgr, out=out, ensemble=ensemble)

    def forward_u8(self, frame, *, bgr: bool = False, out=None, ensemble: int = 1):
        """8-bit frames in, 8-bit frames out, all on the device: `frame` is an (h,w,3) or (B,h,w,3) uint8 device tensor of ANY
        size whose reflect-padding to the next window multiple is defined (padding smaller than the frame); returns
        (B,s*h,s*w,3) uint8.  Equal to the reference's pipeline float32(u8)/255 -> HATModel.pre_process (reflect-pad bottom /
        right) -> forward -> post_process (crop) -> tensor2img, bit for bit against this build's `forward`.  bgr=True: the
        bytes are B,G,R on both sides (OpenCV's order); out: a (B,s*h,s*w,3) uint8 device tensor to fill instead of a fresh
        one (with it the call allocates nothing where conv_last converts in its epilogue).  The padded fp32 input lives in the engine's per-shape workspace.
        Runs eagerly also with use_graph=True (the 8-bit path is not captured).
        ensemble 2 / 4 / 8: pad -> `forward_ensemble` of the padded planes -> crop -> hat_planes_to_u8 (the reference's order of
        pre_process / process / post_process); ensemble=1 is the call as it always was."""
        self._check_u8_input(frame)
        if frame.dim() == 3:
            frame = frame.unsqueeze(0)
        with torch.no_grad():
            return self.engine(frame.device).forward_u8(frame, bgr=bgr, out=out, ensemble=ensemble)

    def forward_gt_u8(self, gt, *, bgr: bool = False, out=None, ensemble: int = 1):
        """Ground-truth frames in, the super-resolution of their own bicubic low-resolution image out, all on the device: `gt`
        is an (H,W,3) or (B,H,W,3) uint8 device tensor; it is mod-cropped to multiples of `upscale` (a view), resized at
        1 / upscale by the reference's MATLAB-style `imresize` (super_resolution_amd/resize.py, bit for bit; float, unrounded,
        as hat/data/imagenet_paired_dataset.py:59 makes its LQ) into the reflect-padded input, and run as forward_u8 runs:
        returns (B, H - H % s, W - W % s, 3) uint8, to be scored against the same mod-cropped `gt`.  bgr, out, ensemble: as
        forward_u8."""
        if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8:
            raise RuntimeError(f"forward_gt_u8 needs a uint8 device tensor, got {getattr(gt, 'dtype', type(gt).__name__)}")
        self._check_u8_input(gt)
        if gt.dim() == 3:
            gt = gt.unsqueeze(0)
        with torch.no_grad():
            return self.engine(gt.device).forward_gt_u8(gt, bgr=bgr, out=out, ensemble=ensemble)

    def forward_yuv420(self, frame, *, fmt: str = "nv12", matrix: str = "bt601", full_range: bool = False, depth: int = 8, out_depth=None,
                       msb=None, out=None, ensemble: int = 1, siting: str = "center", out_siting=None):
        """4:2:0 YCbCr frames in, 4:2:0 frames out, all on the device: `frame` is a (3h/2, w) or (B, 3h/2, w) uint8 device tensor in
        the standard contiguous layout of `fmt` ('nv12', 'nv21', 'i420': super_resolution_amd/yuv.py), h and w even and of ANY
        size whose reflect-padding to the next window multiple is defined; returns (B, 3sh/2, sw) uint8 in the same layout.
        Equal, bit for bit, to yuv.yuv420_to_planes (nearest chroma, `matrix` 'bt601' / 'bt709' / 'bt2020nc', limited or full
        range) -> reflect-pad -> this build's `forward` -> crop -> yuv.planes_to_yuv420 (2 x 2 box chroma).  out: a (B, 3sh/2,
        sw) device tensor to fill instead of a fresh one (with it the call allocates nothing where conv_last converts in its
        epilogue).  depth 10 / 12 / 16: the frame is a uint16 tensor of n-bit codes (P010 / P012 / P016 for nv12 / nv21,
        yuv420p10le ... for i420; msb=True / False overrides the alignment); out_depth (default: depth) is the width of the
        result, uint8 for 8 and uint16 otherwise, so 8 -> 10 writes ten bits from an 8-bit source.  The input dtype must agree
        with `depth`.  No transfer function is applied.  Runs eagerly also with use_graph=True (the byte paths are not captured).
        ensemble 2 / 4 / 8: the padded RGB planes go through `forward_ensemble`, then crop and yuv.planes_to_yuv420
        (hat_planes_to_yuv420); ensemble=1 is the call as it always was.  siting / out_siting: as forward_yuv takes them;
        siting="center" is the call as it always was."""
        if not isinstance(frame, torch.Tensor):
            raise TypeError(f"forward_yuv420 needs a uint8 device tensor, got {type(frame).__name__}")
        if frame.dtype not in (torch.uint8, torch.uint16):
            raise TypeError(f"forward_yuv420 needs a uint8 tensor (uint16 with depth 10, 12 or 16), got {frame.dtype}")
        self._check_u8_input(frame)
        from .. import yuv
        yuv.check_fmt(fmt)
        yuv.csc(matrix, full_range, depth), yuv.csc(matrix, full_range, depth if out_depth is None else out_depth)   # (refused in this order)
        if frame.dtype != (torch.uint8 if depth == 8 else torch.uint16):
            raise TypeError(f"forward_yuv420: depth={depth} needs a {'uint8' if depth == 8 else 'uint16'} tensor, got {frame.dtype}")
        if frame.dim() == 2:
            frame = frame.unsqueeze(0)
        yuv.frame_size(frame.shape)   # (what is no 4:2:0 frame is refused in those words)
        return self.forward_yuv(frame, fmt=fmt, out_fmt=fmt, matrix=matrix, full_range=full_range, depth=depth, out_depth=out_depth, msb=msb,
                                out_msb=msb, out=out, ensemble=ensemble, siting=siting, out_siting=out_siting)

    def forward_yuv(self, frame, *, fmt: str, out_fmt=None, matrix: str = "bt601", full_range: bool = False, depth: int = 8, out_depth=None,
                    msb=None, out_msb=None, out=None, ensemble: int = 1, siting: str = "center", out_siting=None, width=None):
        """YCbCr frames of any chroma subsampling in, any out, all on the device: `frame` is a (rows, w) or (B, rows, w) uint8
        (uint16 with depth 10 / 12 / 16) device tensor in the standard contiguous layout of `fmt`, one of yuv.ALL_FORMATS —
        'nv12' 'nv21' 'i420' (4:2:0), 'i422' 'nv16' (4:2:2), 'i444' 'nv24' (4:4:4), 'gray' — and the result is the s-times larger
        frame in the layout `out_fmt` (default: fmt): nv12 -> i444 keeps all of the network's chroma, i444 -> gray keeps none,
        gray -> i420 writes neutral-born chroma.  w is even where the layout subsamples horizontally and h where vertically;
        every other size >= 1 whose reflect-padding to the next window multiple is defined is a frame.  Equal, bit for bit, to
        yuv.yuv_to_planes -> reflect-pad -> this build's `forward` -> crop -> yuv.planes_to_yuv.  depth / out_depth, matrix,
        full_range, out, ensemble: as forward_yuv420; msb / out_msb: the word alignment of each deep side (default: by the layout).
        forward_yuv420 is this call with out_fmt = fmt for the three 4:2:0 layouts.
        siting: where the source's chroma samples lie (yuv.SITINGS, yuv.py "Chroma siting"): 'center' (JPEG, MPEG-1; nearest up,
        box down: the call as it always was), 'left' (MPEG-2, H.264, HEVC, AV1 4:2:0 and all standard 4:2:2) or 'topleft'
        (BT.2020); out_siting: the result's (None: the input's).  A siting applies to the subsampled axes only, so it is
        ignored by 4:4:4 and grey.  The call stays bit-equal to the composition with the same siting= on both yuv.py functions;
        an output with a co-sited axis is written from fp32 planes (hat_planes_to_yuv_sited), not in conv_last's epilogue.
        Packed 4:2:2: fmt and out_fmt also take yuv.PACKED_FORMATS, in any combination with the layouts above — 'uyvy' and 'yuy2'
        (depth 8, (h, 2w) uint8), 'y210' (depth 10 / 12 / 16, (h, 2w) uint16, MSB-aligned by default) and 'v210' (depth 10, (h, 128
        ceil(w / 48)) uint8; width= is required, ValueError without it: the array does not give it).  The samples mean what 'i422'
        samples mean (yuv.packed_to_planes / planes_to_packed) and the result equals the 'i422' call on the unpacked frame, repacked.
        A packed output is written from fp32 planes (hat_planes_to_packed422).  Standard 4:2:2 video is siting='left'."""
        if not isinstance(frame, torch.Tensor):
            raise TypeError(f"forward_yuv needs a uint8 device tensor, got {type(frame).__name__}")
        if frame.dtype not in (torch.uint8, torch.uint16):
            raise TypeError(f"forward_yuv needs a uint8 tensor (uint16 with depth 10, 12 or 16), got {frame.dtype}")
        self._check_u8_input(frame)
        from .. import ops, yuv
        out_siting = siting if out_siting is None else out_siting
        out_depth = depth if out_depth is None else out_depth
        src = ops.FrameSide(fmt, depth=depth, msb=msb, siting=siting)   # (refuses what is no layout, depth or siting)
        ops.FrameSide(fmt if out_fmt is None else out_fmt, depth=out_depth, msb=out_msb, siting=out_siting)
        to_rgb, from_rgb = yuv.csc(matrix, full_range, depth)[0], yuv.csc(matrix, full_range, out_depth)[1]
        if frame.dtype != src.dtype:
            raise TypeError(f"forward_yuv: depth={depth} {fmt} needs a {str(src.dtype)[6:]} tensor, got {frame.dtype}")
        if fmt == "v210" and width is None:
            raise ValueError("forward_yuv: a v210 frame does not give its width (a row is 128 ceil(w / 48) bytes): pass width=")
        if frame.dim() == 2:
            frame = frame.unsqueeze(0)
        with torch.no_grad():
            return self.engine(frame.device).forward_yuv(frame, fmt=fmt, out_fmt=out_fmt, to_rgb=to_rgb, from_rgb=from_rgb, out=out,
                                                         depth=depth, out_depth=out_depth, msb=msb, out_msb=out_msb, ensemble=ensemble,
                                                         siting=siting, out_siting=out_siting, width=width)

    # ---- exact full-frame sharding into row bands (no counterpart in the reference, whose tile loop
    # hat_model.py:40-108 gives a DIFFERENT result than the full frame: SURVEY F6) ----
    def _check_band_input(self, x):
        if self.training:
            raise RuntimeError("this HAT implements the inference forward pass only: call .eval() first")
        if not x.is_cuda:
            raise RuntimeError("HAT.forward needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")

    def forward_bands(self, x, n_bands: int):
        """`forward(x)` computed as n_bands row bands on this GPU that exchange halo rows and pool sums: equal to the
        unsharded forward up to the summation order of the global pools (band_parallel.forward_bands_local).  Every variant:
        HAT and HATX (SGFN, focus bias, top-k, odd key windows), OCAB-ESC, ape, resi_connection '1conv' / 'identity',
        patch_norm on / off.  Raises RuntimeError when a band would need ghost rows its neighbours do not own (the network's
        deepest refresh, HATEngine.band_halo(): 8 rows for HAT, up to 13 for HATX's live config)."""
        from .. import band_parallel
        self._check_band_input(x)
        with torch.no_grad():
            return band_parallel.forward_bands_local(self.engine(x.device), x, n_bands).to(x.dtype)

    def forward_band_parallel(self, x, group=None):
        """`forward(x)` with one row band per rank of `group` (torch.distributed; RCCL send / recv of halo rows between
        neighbours, one small all-reduce per pool, one all-gather of the output rows): every rank passes the same x and
        receives the full output frame (band_parallel.forward_band_distributed).  The variants and the geometry limit of
        forward_bands apply."""
        from .. import band_parallel
        self._check_band_input(x)
        with torch.no_grad():
            return band_parallel.forward_band_distributed(self.engine(x.device), x, group).to(x.dtype)

    def _forward_graph(self, x):
        """Replay the whole forward (about 290 launches on two streams) as one HIP graph: captured once per input
        shape after two eager warm-up passes, input copied into the graph's static buffer, output copied out of it.
        Removes the host launch path and most inter-kernel gaps; matters most for small frames / tiles.
        The FP16-range guard of HATEngine's residual stream: the guarded launches and the copy of the guard's word
        are part of the graph; the engine zeroes the word before a replay and looks at it behind one, as around an eager
        forward.  Whether the stream is FP16 is part of the cache key: after a fallback the shape is captured again on the fp32
        plan, and the graphs of the old plan are dropped."""
        eng = self.engine(x.device)
        if self._graph_engine is not eng:
            self._graphs, self._graph_engine = collections.OrderedDict(), eng
        guarded = getattr(eng, "_guard", None) is not None
        with torch.cuda.device(x.device):
            if guarded:
                with eng._lock:
                    eng._guard_begin()          # (may find that an earlier frame clipped, and leave the FP16 stream)
            t16 = bool(getattr(eng, "t16", False))
            key = (tuple(x.shape), x.dtype, t16, guarded and eng.t16_guard != "off")   # (a graph holds guarded launches or it does not)
            for k in [k for k in self._graphs if k[2] != t16]:
                del self._graphs[k]
            ent = self._graphs.get(key)
            if ent is None:
                sx = x.detach().clone()
                cur = torch.cuda.current_stream(x.device)
                side = torch.cuda.Stream(device=x.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    for _ in range(2):
                        eng.forward(sx)
                cur.wait_stream(side)
                if bool(getattr(eng, "t16", False)) != t16:   # (a warm-up pass fell back: capture the new plan)
                    return self._forward_graph(x)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    sy = eng.forward(sx)
                # the graph bakes in raw pointers into the engine's workspace of this shape: the entry keeps that
                # workspace alive even after the engine's own LRU has dropped it
                ent = self._graphs[key] = (g, sx, sy, eng._workspace(*x.shape[:1], *x.shape[2:]))
                while len(self._graphs) > self._graph_max:
                    self._graphs.popitem(last=False)
                if guarded:
                    with eng._lock:
                        eng._guard_begin()      # (the warm-up passes ended their own brackets)
                    if bool(getattr(eng, "t16", False)) != t16:   # (their word was looked at here and the engine fell back: the
                        return self._forward_graph(x)             # graph just captured is of the old plan — capture the new one)
            else:
                self._graphs.move_to_end(key)
            g, sx, sy, _ = ent
            sx.copy_(x)
            g.replay()
            y = sy.to(x.dtype, copy=True)
            if guarded:
                with eng._lock:
                    again = eng._guard_end()    # "sync": waits; True: this frame clipped and the engine has fallen back
                if again:
                    return self._forward_graph(x)
            return y


@ARCH_REGISTRY.register()
class HATX(HAT):
    """Drop-in for the reference's `hat.archs.hatx_arch.HATX` (hatx_arch.py:707-974): `HAT` with the Spatial-Gate DConv FFN
    (SGFN) in every HAB and an OCAB that pads its key windows with ceil((wse - ws) / 2), may add a focus bias to the logits
    and may prune keys (top-k).  Same constructor keywords (`hab_ffn_ratio` is accepted and, exactly like the reference,
    never used: its AttenBlocks hands `mlp_ratio` to the HABs, hatx_arch.py:513), same `state_dict()` surface.

    The MI355X forward covers the SGFN, the focus bias and the top-k pruning for key windows of 12 / 24 (overlap 0.5) and the
    odd 13 / 25 (ceil padding, hatx_arch.py:303-305: overlap 0.7 at window 8, 0.6 at window 16 — the live training config, in
    bf16), ESC on up to 32 channels with kernels up to 17 x 17.  Among keys of EQUAL score the pruning keeps the lower window index, where the reference
    leaves the order to torch.topk: border windows, whose zero-padded keys all score tanh(0) = 0, can therefore differ from
    the reference; windows without padded keys cannot.
    """
    _VARIANT = "hatx"

    def __init__(self, *args, hab_ffn_ratio: float = 2.0, kv_topk_ratio: float = 1.0, use_focus_bias: bool = False, **kwargs):
        self.hab_ffn_ratio = hab_ffn_ratio
        super().__init__(*args, _kv_topk_ratio=kv_topk_ratio, _use_focus_bias=use_focus_bias, **kwargs)
        self.kv_topk_ratio, self.use_focus_bias = float(kv_topk_ratio), bool(use_focus_bias)
