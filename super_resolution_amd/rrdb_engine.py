"""`RRDBEngine` — RRDBNet (rrdbnet_arch.py:66-119) as a launch sequence on the MI355X: packed weights, a workspace per input shape,
no torch op on the hot path.  DESIGN.md §4.26 has the launch list.

    [hat_unshuffle_pad (scale 2 / 1: PixelUnshuffle(2 / 4) -> fp32 rows of 12 / 48 channels)]
    hat_conv   conv_first -> feat, fp32 rows: the head of the fp32 residual stream
    hat_conv   1x1 identity: feat rounded once to T into channels [0,64) of the first dense buffer            (bf16 only)
    per RDB    4 x hat_rdb_conv in place (conv k stores x_k at channel 64 + 32 (k - 1) of the block's dense rows),
               hat_rdb_conv conv 5: 0.2 (conv + bias) + the RDB's input [, x 0.2 + the RRDB's input] -> the next fp32 stream buffer and,
               rounded to T, channels [0,64) of the OTHER dense buffer
    hat_conv   conv_body + feat -> n
    esc_parts.NearestX4Head's four launches: conv_up1 / conv_up2 folded with their nearest x2 steps, conv_hr, conv_last -> planes
    or the fused byte / YCbCr sink.
The fp32 compute path runs the dense layers on hat_conv (hat_rdb_conv has no fp32 instantiation): channels [0,64) come from the
fp32 stream itself (x0 / c_split), so one dense buffer serves; 0.2 (0.04 for the third block) is folded into conv 5's packed
weights and bias, r1 is the stream and r2 / r2scale carry the third block's 0.2 x term."""
from __future__ import annotations

import torch

from . import ops
from .engine_base import EngineBase
from .esc_parts import NearestX4Head
from .frame_boundary import FrameBoundary
from .ops import ACT_LRELU02, O_NHWC_F32, X_NCHW_F32_MEAN, X_NHWC_F32

BUILT = "num_feat 64, num_grow_ch 32, num_in_ch = num_out_ch = 3, scale 1, 2 or 4, any num_block >= 0"
SLOPE, BETA = 0.2, 0.2        # nn.LeakyReLU(0.2) (rrdbnet_arch.py:27); the residual scale of :39 and :62
LD = 192                      # channels of a dense row: 64 + 4 x 32
# the dense layers hat_rdb_conv runs in bf16 (the others go to hat_conv): all five, profiles/rrdb_path.txt
RDB_KERNEL_CIN = frozenset(ops.RDB_CIN)


def check_cfg(cfg):
    nb, s = cfg["num_block"], cfg["scale"]
    ok = (int(cfg["num_feat"]) == 64 and int(cfg["num_grow_ch"]) == 32 and int(cfg["num_in_ch"]) == 3 and int(cfg["num_out_ch"]) == 3
          and s in (1, 2, 4) and int(nb) == nb and nb >= 0)
    if not ok:
        raise ValueError("RRDBNet with " + ", ".join(f"{k}={cfg[k]!r}" for k in ("num_in_ch", "num_out_ch", "scale", "num_feat", "num_block",
                                                                                 "num_grow_ch"))
                         + f" is not supported: the device path is built for {BUILT}")


class RRDBEngine(FrameBoundary, EngineBase):
    """The frame boundary (frame_boundary.FrameBoundary) is mixed in as it is for SRVGGEngine.  At scale 2 / 1 the network unshuffles
    by f = 2 / 4: `forward` refuses a frame that f does not divide, as the reference does; the frame calls reflect-pad to a multiple
    of f and crop, as Real-ESRGAN's inference wrapper does."""
    WS_MAX = 4   # entries of the workspace LRU

    def __init__(self, cfg: dict, sd: dict, device, compute_dtype: str = "bf16"):
        check_cfg(cfg)
        if compute_dtype not in ops.DTYPE_CODE:
            raise ValueError(f"compute_dtype {compute_dtype!r}: expected 'bf16' or 'fp32'")
        super().__init__(device, compute_dtype, self.WS_MAX)   # (a host device is taken: the engine then packs and never runs)
        self.cfg = dict(cfg, in_chans=3)
        self.u8_fused_calls = self.u8_planes_calls = 0   # 8-bit forwards that ended in hat_conv3x3_to_u8 / in hat_planes_to_u8
        self.yuv_fused_calls = self.yuv_planes_calls = 0   # YCbCr forwards that ended in hat_conv3x3_to_yuv / in a from-planes kernel
        self.C, self.scale, self.ws, self.nb = 64, int(cfg["scale"]), 1, int(cfg["num_block"])
        self.f = 4 // self.scale                         # the unshuffle factor: 1, 2, 4
        self.bf16 = self.dtype == ops.HAT_BF16
        dt, dev = self.dtype, self.dev
        conv = lambda name, **kw: ops.pack_conv_weight(sd[name + ".weight"], sd[name + ".bias"], dt, dev, **kw)
        self.first, self.last = conv("conv_first"), conv("conv_body")
        self.ident = ops.pack_conv_weight(torch.eye(64)[:, :, None, None], None, dt, dev) if self.bf16 else None
        self.blocks = []   # per RRDB, per RDB: the five packed convs
        for i in range(self.nb):
            rrdb = []
            for r in (1, 2, 3):
                p, rdb = f"body.{i}.rdb{r}.conv", []
                for k in range(1, 6):
                    cin = 64 + 32 * (k - 1)
                    if self.bf16 and cin in RDB_KERNEL_CIN:
                        rdb.append(ops.pack_rdb_conv(sd[f"{p}{k}.weight"], sd[f"{p}{k}.bias"], dt, dev))
                    else:   # conv 5: beta folded (beta^2 where the RRDB's own residual follows)
                        rdb.append(conv(f"{p}{k}", scale=1.0 if k < 5 else (BETA * BETA if r == 3 else BETA)))
                rrdb.append(rdb)
            self.blocks.append(rrdb)
        self.head = NearestX4Head(self, {f"to_img.{i}.{k}": sd[f"{n}.{k}"] for i, n in ((1, "conv_up1"), (4, "conv_up2"), (6, "conv_hr"), (8, "conv_last"))
                                         for k in ("weight", "bias")})

    def _pad_multiple(self) -> int:
        return self.f

    def _body_size(self, h: int, w: int):
        return h // self.f, w // self.f

    def _alloc_workspace(self, B: int, h: int, w: int, tag=None):
        H, W = self._body_size(h, w)
        dev, N = self.dev, H * W
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        t = lambda *shape: torch.zeros(*shape, dtype=self.tdt, device=dev)
        ws = {"feat": f(B, N, 64), "s": [f(B, N, 64) for _ in range(3)], "d": [t(B, N, LD) for _ in range(2 if self.bf16 else 1)], "n": t(B, N, 64),
              "beta": torch.full((B, 64), BETA, dtype=torch.float32, device=dev)}
        if self.f > 1:
            ws["xr"] = f(B, N, 3 * self.f ** 2)
        ws.update(self.head.buffers(B, H, W, f, t))
        return ws

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
            raise RuntimeError(f"RRDBNet expects (B,3,h,w) input with B, h, w >= 1, got {tuple(x.shape)}")
        h, w = x.shape[2:]
        assert h % self.f == 0 and w % self.f == 0, (f"RRDBNet at scale {self.scale} unshuffles the frame by {self.f}: a {h}x{w} frame is not "
                                                     f"divisible by it (the frame calls upscale_u8 / upscale_yuv pad and crop)")

    def _rdb(self, rdb, r, w, d, dn, r1, r2, s_out, geo):
        """One residual dense block: d the block's dense rows, dn the next block's, r1 the block's input on the fp32 stream, r2 the
        RRDB's input (third block only), s_out the stream buffer behind the block."""
        dt = self.dtype
        for k, pw in enumerate(rdb, 1):
            cin = 64 + 32 * (k - 1)
            if isinstance(pw, ops.PackedRdbConv):
                if k < 5:
                    ops.rdb_conv(pw, d, d, **geo, dtype=dt, ldx=LD, ldo=LD, out_off=cin, slope=SLOPE)
                else:
                    ops.rdb_conv(pw, d, dn, **geo, dtype=dt, ldx=LD, ldo=LD, out_off=0, beta1=BETA, beta2=BETA, r1=r1, r2=r2, s_out=s_out)
                continue
            # hat_conv: in bf16 the block's input is in d like the rest; in fp32 it is the stream itself
            src = {} if self.bf16 else dict(x0=r1, c_split=64, ldx0=64)
            if k < 5:
                ops.conv(pw, d, d.view(-1)[cin:], **geo, dtype=dt, ldx=LD, ldo=LD, act=ACT_LRELU02, n_store=32, **src)
                continue
            res = dict(r1=r1, ldr1=64) if r2 is None else dict(r1=r2, ldr1=64, r2=self._as_t(r1, w), ldr2=64, r2scale=w["beta"], r2scale_bstride=64)
            ops.conv(pw, d, s_out, **geo, dtype=dt, ldx=LD, ldo=64, out_mode=O_NHWC_F32, **src, **res)
            if self.bf16:
                ops.conv(self.ident, s_out, dn, **geo, dtype=dt, ldx=64, ldo=LD, x_mode=X_NHWC_F32, n_store=64)

    def _as_t(self, rows, w):
        """hat_conv's r2 is T rows: in fp32 the stream itself.  (In bf16 conv 5 always runs on hat_rdb_conv, whose r2 is fp32.)"""
        if self.bf16:
            raise RuntimeError("RRDBEngine: conv 5 of the third block has no hat_conv route in bf16 (its r2 is an fp32 stream)")
        return rows

    def _forward(self, x: torch.Tensor, one_stream=None, sink=None, taps: dict = None) -> torch.Tensor:
        """x (B, 3, h, w) fp32 -> (B, 3, s h, s w) fp32 (the workspace's output buffer: copy it before the next forward of the shape).
        one_stream: accepted and ignored (there is no side stream).  sink (a frame_boundary._Sink): the head fills and returns
        sink.out instead of fp32 planes.  taps: a dict that receives a clone of the fp32 stream behind every RRDB, under its index."""
        self._check_input(x)
        B, _, h, wd = x.shape
        H, W = self._body_size(h, wd)
        x = x.to(torch.float32).contiguous()
        w, dt = self._workspace(B, h, wd), self.dtype
        geo = dict(B=B, H=H, W=W)
        feat = w["feat"]
        if self.f == 1:
            ops.conv(self.first, x, feat, **geo, dtype=dt, ldx=0, ldo=64, x_mode=X_NCHW_F32_MEAN, out_mode=O_NHWC_F32)
        else:
            cin = 3 * self.f ** 2
            ops.unshuffle_pad(x, w["xr"], B=B, h=h, w=wd, f=self.f, ld=cin)
            ops.conv(self.first, w["xr"], feat, **geo, dtype=dt, ldx=cin, ldo=64, x_mode=X_NHWC_F32, out_mode=O_NHWC_F32)
        d = w["d"][0]
        dn = w["d"][1] if self.bf16 else d
        if self.bf16 and self.nb:
            ops.conv(self.ident, feat, d, **geo, dtype=dt, ldx=64, ldo=LD, x_mode=X_NHWC_F32, n_store=64)
        cur = feat
        for i, rrdb in enumerate(self.blocks):
            a, b = [s for s in w["s"] if s is not cur][:2]
            self._rdb(rrdb[0], 1, w, d, dn, cur, None, a, geo)
            self._rdb(rrdb[1], 2, w, dn, d, a, None, b, geo)
            self._rdb(rrdb[2], 3, w, d, dn, b, cur, a, geo)
            d, dn, cur = dn, d, a
            if taps is not None:
                taps[i] = cur.clone()
        return self.head.run(x, w, cur, feat, geo, sink=sink)
