"""`SRVGGEngine` — SRVGGNetCompact (srvgg_arch.py:6-69) as a launch sequence on the MI355X: packed weights, a workspace per input
shape, no torch op on the hot path.  DESIGN.md §4.25 has the launch list.

    hat_vgg_conv (frame mode: the fp32 planes -> 64-channel T rows, + activation)
    num_conv x hat_vgg_conv (rows -> rows, + activation; two buffers, ping-pong)
    hat_conv 64 -> 3 s^2 (fp32 rows, padded to a multiple of 4 with zero weight rows)
    hat_esc_shuffle_add (PixelShuffle(s) + the nearest-upsampled input) | hat_shuffle_to_u8 | hat_shuffle_to_yuv into a frame
The activation is a slope vector on the negative side: the PReLU weights, zeros (ReLU) or 0.1 (the reference's LeakyReLU)."""
from __future__ import annotations

import torch

from . import ops
from .engine_base import EngineBase
from .frame_boundary import FrameBoundary
from .ops import O_NHWC_F32

ACT_TYPES = ("relu", "prelu", "leakyrelu")
BUILT = "num_feat 64, num_in_ch = num_out_ch = 3, upscale 1..4, any num_conv >= 0, act_type 'relu' | 'prelu' | 'leakyrelu'"


def _r4(n: int) -> int:
    return (n + 3) // 4 * 4


def check_cfg(cfg):
    nc, s = cfg["num_conv"], cfg["upscale"]
    ok = (int(cfg["num_feat"]) == 64 and int(cfg["num_in_ch"]) == 3 and int(cfg["num_out_ch"]) == 3 and cfg["act_type"] in ACT_TYPES
          and int(s) == s and 1 <= s <= 4 and int(nc) == nc and nc >= 0)
    if not ok:
        raise ValueError("SRVGGNetCompact with " + ", ".join(f"{k}={cfg[k]!r}" for k in ("num_in_ch", "num_out_ch", "num_feat", "num_conv",
                                                                                        "upscale", "act_type"))
                         + f" is not supported: the device path is built for {BUILT}")


class SRVGGEngine(FrameBoundary, EngineBase):
    """The frame boundary (frame_boundary.FrameBoundary) is mixed in as it is for ESCEngine: a frame of any size >= 1x1 is taken
    unpadded, batches are taken, and the head ends in the shuffle sinks where the sink can take them."""
    WS_MAX = 4   # entries of the workspace LRU

    def __init__(self, cfg: dict, sd: dict, device, compute_dtype: str = "bf16"):
        check_cfg(cfg)
        if compute_dtype not in ops.DTYPE_CODE:
            raise ValueError(f"compute_dtype {compute_dtype!r}: expected 'bf16' or 'fp32'")
        super().__init__(device, compute_dtype, self.WS_MAX)   # (a host device is taken: the engine then packs and never runs)
        self.cfg = dict(cfg, in_chans=3)
        self.u8_fused_calls = self.u8_planes_calls = 0   # 8-bit forwards that ended in hat_shuffle_to_u8 / in hat_planes_to_u8
        self.yuv_fused_calls = self.yuv_planes_calls = 0   # YCbCr forwards that ended in hat_shuffle_to_yuv / in a from-planes kernel
        self.C, self.scale, self.ws, n = 64, int(cfg["upscale"]), 1, int(cfg["num_conv"])
        dt, dev, act = self.dtype, self.dev, cfg["act_type"]

        def slope(i):
            if act == "prelu":
                return sd[f"body.{2 * i + 1}.weight"]
            return torch.full((64,), 0.1 if act == "leakyrelu" else 0.0)

        self.layers = [ops.pack_vgg_conv(sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"], slope(i), dt, dev) for i in range(n + 1)]
        self.last = ops.pack_conv_weight(sd[f"body.{2 * n + 2}.weight"], sd[f"body.{2 * n + 2}.bias"], dt, dev)
        self.ld = _r4(3 * self.scale ** 2)

    def _pad_multiple(self) -> int:
        return 1   # any frame size is taken as it is

    def _alloc_workspace(self, B: int, H: int, W: int, tag=None):
        dev, s = self.dev, self.scale
        return {"t": [torch.zeros(B, H * W, 64, dtype=self.tdt, device=dev) for _ in range(2)],
                "rows": torch.zeros(B, H * W, self.ld, dtype=torch.float32, device=dev),
                "y": torch.zeros(B, 3, H * s, W * s, dtype=torch.float32, device=dev)}

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
            raise RuntimeError(f"SRVGGNetCompact expects (B,3,h,w) input with B, h, w >= 1, got {tuple(x.shape)}")

    def _forward(self, x: torch.Tensor, one_stream=None, sink=None, taps: dict = None) -> torch.Tensor:
        """x (B, 3, h, w) fp32 -> (B, 3, s h, s w) fp32 (the workspace's output buffer: copy it before the next forward of the shape).
        one_stream: accepted and ignored (there is no side stream).  sink (a frame_boundary._Sink): the head fills and returns
        sink.out instead of fp32 planes.  taps: a dict that receives a clone of the rows behind every layer, under its index."""
        self._check_input(x)
        B, _, H, W = x.shape
        x = x.to(torch.float32).contiguous()
        w, dt, s = self._workspace(B, H, W), self.dtype, self.scale
        geo = dict(B=B, H=H, W=W)
        cur, nxt = w["t"]
        for i, pv in enumerate(self.layers):
            ops.vgg_conv(pv, x if i == 0 else cur, cur if i == 0 else nxt, **geo, dtype=dt)
            if i:
                cur, nxt = nxt, cur
            if taps is not None:
                taps[i] = cur.clone()
        ops.conv(self.last, cur, w["rows"], **geo, dtype=dt, ldx=64, ldo=self.ld, out_mode=O_NHWC_F32, n_store=self.ld)
        if sink is not None and sink.fusable:   # rows + base image straight to the frame: w["y"] is not written
            sink.shuffled(w["rows"], x, **geo, s=s, ld=self.ld)
            return sink.out
        ops.esc_shuffle_add(w["rows"], x, w["y"], **geo, s=s, ld=self.ld)
        if sink is None:
            return w["y"]
        sink.from_planes(w["y"])
        return sink.out
