"""`ESCLTE` — the ESC paper's arbitrary-scale model (the reference's ESC/esc_arb: `models/lte.py:LTE` over `models/esc.py:Net`,
configs/train-div2k/train_esc-lte.yaml): an ESC encoder without `to_img`, and the Local Texture Estimator, which evaluates an MLP on a
Fourier basis built from the four nearest feature pixels for ANY output coordinate.  Same `state_dict()` surface as the reference's
`LTE`, key for key; `from_checkpoint` takes the reference's checkpoint dict.  The module tree only holds parameters:
`ESCLTEEngine` (esc_engine.py) runs the encoder's launches and `hat_lte_query` on the MI355X.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY
from .esc_arch import _Block, _ESCNet
from .hat_arch import HAT, _Holder


class _Encoder(_Holder):  # esc_arb/models/esc.py:255-296
    def __init__(self, dim, pdim, kernel_size, n_blocks, conv_blocks, window_size, num_heads, exp_ratio):
        super().__init__()
        self.plk_filter = nn.Parameter(torch.randn(pdim, pdim, kernel_size, kernel_size))
        torch.nn.init.orthogonal_(self.plk_filter)
        self.proj = nn.Conv2d(3, dim, 3, 1, 1)
        self.blocks = nn.ModuleList([_Block(dim, pdim, conv_blocks, window_size, num_heads, exp_ratio, False) for _ in range(n_blocks)])
        self.last = nn.Conv2d(dim, dim, 3, 1, 1)


class _MLP(_Holder):  # esc_arb/models/mlp.py:7-23
    def __init__(self, in_dim, out_dim, hidden_list):
        super().__init__()
        layers, lastv = [], in_dim
        for hidden in hidden_list:
            layers += [nn.Linear(lastv, hidden), nn.ReLU()]
            lastv = hidden
        layers.append(nn.Linear(lastv, out_dim))
        self.layers = nn.Sequential(*layers)


@ARCH_REGISTRY.register()
class ESCLTE(_ESCNet):
    """ESC-LTE on the MI355X.  Everything from the engine up is the ESC family's (and through it `HAT`'s): `compute_dtype` /
    `set_compute_dtype`, the weight-change tracking.

    Calls, in the reference's normalised domain (the caller applies `data_norm`):
      gen_feat(inp)              inp (1,3,H,W): the encoder and the coef / freq convs; -> the feature map (1,64,H,W) fp32
      query_rgb(coord, cell)     (1,Q,2) fp32 device tensors, (y, x) order, coord in [-1, 1] -> (1,Q,3) fp32 against the last gen_feat
      forward(inp, coord, cell)  the two together (the reference's `batched_predict` and `model(inp, coord, cell)`)
      upscale(img, size= | scale=, scale_max=4)   img (1,3,H,W) in [0, 1] -> (1,3,h,w) fp32, not clamped: inference.py:64-73 with
                                 the coordinates and cells made inside the kernel
    `query_rgb` and `upscale` run eagerly also with `use_graph=True`: a query's size is the caller's, there is nothing to replay;
    `gen_feat` runs eagerly as well.

    Built: the encoder of train_esc-lte.yaml (dim 64, pdim 16, kernel_size 13, window_size 32, num_heads 4, exp_ratio 1.25 or 2,
    any n_blocks / conv_blocks), hidden_dim 256, hidden_list (256, 256, 256); anything else is a ValueError when the engine packs.
      upscale_u8(frame, size= | scale=)           an (h,w,3) uint8 device frame -> (1,H',W',3) uint8: tensor2img's bytes of `upscale`
      upscale_yuv(frame, size= | scale=, fmt=)    a YCbCr device frame of any layout and depth -> the resized frame in any layout
      score_u8(lr, gt, eval_type=)                a paired LR / GT frame -> the PSNR of the reference's test.py (`benchmark-S`, `div2k-S`)
      score_gt_u8(gt, scale, eval_type=)          a GT frame: the LR frame by Pillow's 8-bit bicubic resize on the device, then the same
    `query_rgb`, the three `upscale` calls and the two `score` calls run eagerly also with `use_graph=True`.
    One frame per call.  `forward_ensemble`, the fixed-scale byte and YCbCr entry points (`forward_u8`, `forward_yuv`, ...), row bands
    and plans raise NotImplementedError, as for `ESC`: this network's frame paths are `upscale_u8` and `upscale_yuv`."""
    arbitrary_scale = True   # frames.upscale_frames: size= / scale= go to upscale_u8 / upscale_yuv; nothing else does

    def __init__(self, dim: int = 64, pdim: int = 16, kernel_size: int = 13, n_blocks: int = 5, conv_blocks: int = 5, window_size: int = 32,
                 num_heads: int = 4, exp_ratio: float = 1.25, hidden_dim: int = 256, hidden_list=(256, 256, 256), compute_dtype: str = "bf16",
                 use_graph: bool = False):
        nn.Module.__init__(self)
        hidden_list = tuple(int(v) for v in hidden_list)
        self.encoder = _Encoder(dim, pdim, kernel_size, n_blocks, conv_blocks, window_size, num_heads, exp_ratio)
        self.coef = nn.Conv2d(dim, hidden_dim, 3, padding=1)
        self.freq = nn.Conv2d(dim, hidden_dim, 3, padding=1)
        self.phase = nn.Linear(2, hidden_dim // 2, bias=False)
        self.imnet = _MLP(hidden_dim, 3, hidden_list)
        self.upscaling_factor = 1   # (what the family's harness sizes by: this network has no fixed scale)
        self.window_size, self.in_chans, self.img_range = int(window_size), 3, 1.0
        self.cfg = dict(dim=dim, pdim=pdim, kernel_size=kernel_size, n_blocks=n_blocks, conv_blocks=conv_blocks, window_size=window_size,
                        num_heads=num_heads, exp_ratio=exp_ratio, use_ln=False, converted=False, hidden_dim=int(hidden_dim),
                        hidden_list=hidden_list)
        self.compute_dtype = compute_dtype
        self._init_runtime(bool(use_graph))

    def _anchor(self) -> torch.Tensor:
        return self.coef.weight

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """A plain load: there is no `to_img` whose scale could be converted."""
        return HAT.load_state_dict(self, state_dict, strict, assign)

    @classmethod
    def from_checkpoint(cls, obj, **kw):
        """The reference's checkpoint dict {'model': {'name': 'lte', 'args': {...}, 'sd': {...}}} (esc_arb/train.py, models.make with
        load_sd).  The encoder is the default one: the reference's `make_swinir` ignores its arguments too."""
        spec = obj["model"] if isinstance(obj, dict) and "model" in obj else obj
        if not isinstance(spec, dict) or spec.get("name") != "lte":
            raise ValueError(f"ESCLTE.from_checkpoint expects a checkpoint of model 'lte', got {spec.get('name') if isinstance(spec, dict) else type(spec).__name__!r}")
        args = spec.get("args", {})
        enc = args.get("encoder_spec", {})
        if enc.get("name") != "esc":
            raise ValueError(f"ESCLTE.from_checkpoint: encoder {enc.get('name')!r} is not supported: only 'esc' is built (DESIGN.md §7)")
        im = args.get("imnet_spec") or {}
        if im.get("name") != "mlp" or int(im.get("args", {}).get("out_dim", 0)) != 3:
            raise ValueError(f"ESCLTE.from_checkpoint: imnet_spec {im!r} is not supported: expected an 'mlp' with out_dim 3")
        net = cls(hidden_dim=int(args.get("hidden_dim", 256)), hidden_list=tuple(im["args"].get("hidden_list", ())), **kw)
        if "sd" in spec:
            net.load_state_dict(spec["sd"], strict=True)
        return net.eval()

    def _make_engine(self, device):
        from ..esc_engine import ESCLTEEngine
        return ESCLTEEngine(self.cfg, self.state_dict(), device, self.compute_dtype)

    # ------------------------------------------------------------------------------------------
    def _check_call(self, inp):
        if self.training:
            raise RuntimeError("this ESC-LTE implements the inference forward pass only: call .eval() first (training is out of scope)")
        if not inp.is_cuda:
            raise RuntimeError("ESCLTE needs a GPU tensor: the MI355X HIP path is the only path (no CPU fallback)")

    def _gen(self, inp):
        self._check_call(inp)
        eng = self.engine(inp.device)
        rows = eng.forward(inp)
        self._feat_engine = eng
        return eng, rows

    def gen_feat(self, inp):
        with torch.no_grad():
            _, rows = self._gen(inp)
            H, W = inp.shape[-2:]
            return rows.reshape(1, H, W, -1).permute(0, 3, 1, 2).to(torch.float32).contiguous()

    def _feat(self):
        eng = getattr(self, "_feat_engine", None)
        if eng is None or eng is not self._engine:
            raise RuntimeError("ESCLTE.query_rgb before gen_feat (or after the weights changed): there are no features to query")
        return eng

    def query_rgb(self, coord, cell):
        eng = self._feat()
        for name, t in (("coord", coord), ("cell", cell)):
            if t.dim() != 3 or t.shape[0] != 1 or t.shape[2] != 2:
                raise RuntimeError(f"ESCLTE.query_rgb expects {name} as (1,Q,2), got {tuple(t.shape)}")
        with torch.no_grad():
            return eng.query(coord[0].to(torch.float32), cell[0].to(torch.float32))[None]

    def forward(self, inp, coord, cell):
        self.gen_feat_only(inp)
        return self.query_rgb(coord, cell)

    def gen_feat_only(self, inp):
        """gen_feat without materialising the returned feature map."""
        with torch.no_grad():
            self._gen(inp)

    def upscale(self, img, size=None, scale=None, scale_max=4):
        if (size is None) == (scale is None):
            raise ValueError("ESCLTE.upscale takes exactly one of size=(h, w) and scale=")
        if img.dim() != 4 or img.shape[1] != 3:
            raise RuntimeError(f"ESCLTE.upscale expects (1,3,H,W) input, got {tuple(img.shape)}")
        H, W = int(img.shape[-2]), int(img.shape[-1])
        h, w = (int(H * scale), int(W * scale)) if size is None else (int(size[0]), int(size[1]))
        if h < 1 or w < 1:
            raise ValueError(f"ESCLTE.upscale: an output of {h}x{w} is empty")
        self._check_call(img)
        with torch.no_grad():
            eng, _ = self._gen((img.to(torch.float32) - 0.5) / 0.5)
            factor = max((h / H) / scale_max, 1)   # inference.py:64, 70: the cell of the largest trained scale
            cy, cx = (float(torch.tensor(2 / n, dtype=torch.float32) * factor) for n in (h, w))   # rounded as the reference rounds them
            return eng.query_grid(h, w, (cy, cx), out_affine=(0.5, 0.5))[None]

    # ---- frames in, frames out: any output size.  New names: the fixed-scale entry points above keep refusing.
    def _out_size(self, what, H, W, size, scale):
        if (size is None) == (scale is None):
            raise ValueError(f"ESCLTE.{what} takes exactly one of size=(h, w) and scale=")
        h, w = (int(H * scale), int(W * scale)) if size is None else (int(size[0]), int(size[1]))
        if h < 1 or w < 1:
            raise ValueError(f"ESCLTE.{what}: an output of {h}x{w} is empty")
        return h, w

    @staticmethod
    def _cells(H, W, h, w, scale_max):
        factor = max((h / H) / scale_max, 1)   # upscale's cell rule (inference.py:64, 70)
        return tuple(float(torch.tensor(2 / n, dtype=torch.float32) * factor) for n in (h, w))

    def upscale_u8(self, frame, size=None, scale=None, *, bgr: bool = False, out=None, scale_max=4):
        """An 8-bit frame in, an 8-bit frame of any size out, all on the device: `frame` (h,w,3) or (1,h,w,3) uint8 -> (1,H',W',3)
        uint8 with (H', W') = size or (int(h scale), int(w scale)).  Equal, bit for bit, to float32(u8) / 255 -> `upscale` ->
        tensor2img (clamp to [0, 1], x255 in fp32, round half to even): hat_u8_to_planes into the workspace (no padding: ESC reflects
        its own window edges), the encoder, and one hat_lte_query_u8, which stores the bytes itself; no fp32 image is written.
        bgr: the bytes are B, G, R on both sides.  out: a (1,H',W',3) uint8 device tensor to fill (rows may be pitched); with it the
        call allocates nothing after the first call of a shape."""
        if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() not in (3, 4) or frame.shape[-1] != 3:
            raise RuntimeError(f"ESCLTE.upscale_u8 expects an (h,w,3) or (1,h,w,3) uint8 frame, got {tuple(getattr(frame, 'shape', ()))} "
                               f"{getattr(frame, 'dtype', type(frame).__name__)}")
        if frame.dim() == 3:
            frame = frame.unsqueeze(0)
        if frame.shape[0] != 1:
            raise RuntimeError(f"ESCLTE.upscale_u8 takes one frame per call, got a batch of {frame.shape[0]}")
        H, W = int(frame.shape[1]), int(frame.shape[2])
        h, w = self._out_size("upscale_u8", H, W, size, scale)
        self._check_call(frame)
        from .. import ops
        with torch.no_grad():
            eng = self.engine(frame.device)
            dst = out
            if dst is None:
                dst = torch.empty((1, h, w, 3), dtype=torch.uint8, device=eng.dev)
            elif not isinstance(dst, torch.Tensor) or dst.dtype != torch.uint8 or tuple(dst.shape) != (1, h, w, 3) or dst.device != eng.dev \
                    or dst.stride(3) != 1 or dst.stride(2) != 3:
                raise RuntimeError(f"out must be a {(1, h, w, 3)} uint8 tensor on {eng.dev} with interleaved pixels, got "
                                   f"{tuple(getattr(dst, 'shape', ()))} {getattr(dst, 'dtype', type(dst).__name__)} on {getattr(dst, 'device', None)}")
            if frame.stride(3) != 1 or frame.stride(2) != 3:
                frame = frame.contiguous()
            eng.gen_feat_frame(H, W, lambda x: ops.u8_to_planes(frame, x, bgr=bgr))
            self._feat_engine = eng
            return eng.query_grid_u8(dst, self._cells(H, W, h, w, scale_max), bgr)

    # ---- the reference's benchmark loop (esc_arb/test.py eval_psnr over the configs/test files): bytes in, a score
    # out.  New names; the arithmetic of sizes, crops and cells is arb_test's, where it runs without a device.
    def _u8_frame(self, what, name, frame):
        if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3:
            raise RuntimeError(f"ESCLTE.{what} expects {name} as an (h,w,3) uint8 frame, got {tuple(getattr(frame, 'shape', ()))} "
                               f"{getattr(frame, 'dtype', type(frame).__name__)}")
        self._check_call(frame)
        return frame if frame.stride(2) == 1 and frame.stride(1) == 3 else frame.contiguous()

    def _score(self, what, eng, lr, gt, eval_type, scale_max):
        from .. import arb_test, ops
        mode, shave, S = arb_test.parse_eval_type(eval_type)
        H, W = int(lr.shape[0]), int(lr.shape[1])
        h, w = int(gt.shape[0]), int(gt.shape[1])
        arb_test.check_lr_size(H, W)
        if 2 * shave >= min(h, w):
            raise ValueError(f"ESCLTE.{what}: eval_type {eval_type!r} shaves {shave} pixels off every side, which leaves nothing of a {h}x{w} ground truth")
        eng.gen_feat_frame(H, W, lambda x: ops.u8_to_planes(lr.unsqueeze(0), x))
        self._feat_engine = eng
        total, terms = eng.score_grid(gt, arb_test.eval_cells(h, w, S, scale_max), mode, shave)
        return arb_test.psnr_of(total, terms)

    def score_u8(self, lr_u8, gt_u8, *, eval_type, scale_max=4):
        """One image of a paired test set (`sr-implicit-paired[-fast]`, esc_arb/datasets/wrappers.py:27-34) scored on the device:
        lr_u8 (h,w,3) and gt_u8 (H,W,3) uint8 device frames -> the reference's PSNR as a Python float.  s = H // h; the ground truth
        is cropped to (h s, w s), which is also the queried grid; the cells are 2 / (h s), 2 / (w s) rounded to fp32, times
        max(S / scale_max, 1) with S the integer of `eval_type` ('benchmark-S': the weighted channel sum, S pixels shaved;
        'div2k-S': all of RGB, S + 6 shaved; None: all of RGB, no shave, the cell as it is; anything else: NotImplementedError).
        hat_u8_to_planes, the encoder, hat_lte_query into the workspace, hat_arb_psnr: only the score leaves the device."""
        from .. import arb_test
        lr, gt = self._u8_frame("score_u8", "lr_u8", lr_u8), self._u8_frame("score_u8", "gt_u8", gt_u8)
        _, (h, w) = arb_test.paired_sizes(lr.shape[0], lr.shape[1], gt.shape[0], gt.shape[1])
        with torch.no_grad():
            return self._score("score_u8", self.engine(lr.device), lr, gt[:h, :w], eval_type, scale_max)

    def score_gt_u8(self, gt_u8, scale, *, eval_type, scale_max=4):
        """One image of a ground-truth-only test set (`sr-implicit-downsampled[-fast]` with inp_size unset, wrappers.py:172-181):
        per axis h_lr = floor(H / scale + 1e-9), the ground truth cropped to round(h_lr scale), the LR frame made from it by Pillow's
        8-bit bicubic resize on the device (hat_pil_resize_u8: the bytes of the reference's `resize_fn`); then as `score_u8`."""
        from .. import arb_test
        gt = self._u8_frame("score_gt_u8", "gt_u8", gt_u8)
        arb_test.parse_eval_type(eval_type)   # refuse before the resize runs
        (h_lr, w_lr), (h, w) = arb_test.downsampled_sizes(gt.shape[0], gt.shape[1], scale)
        arb_test.check_lr_size(h_lr, w_lr)
        with torch.no_grad():
            eng = self.engine(gt.device)
            gt = gt[:h, :w]
            return self._score("score_gt_u8", eng, eng.pil_lr_frame(gt, h_lr, w_lr), gt, eval_type, scale_max)

    def upscale_yuv(self, frame, size=None, scale=None, *, fmt: str, out_fmt=None, matrix: str = "bt601", full_range: bool = False, depth: int = 8,
                    out_depth=None, msb=None, out_msb=None, out=None, siting: str = "center", out_siting=None, scale_max=4, width=None):
        """A YCbCr frame in, a YCbCr frame of any size out, all on the device: `frame` is a (rows, w) or (1, rows, w) uint8 (uint16
        with depth 10 / 12 / 16) device tensor in the standard layout of `fmt` (yuv.LAYOUTS or yuv.PACKED_FORMATS); the result is the
        (H', W') frame in the layout `out_fmt` (default: fmt), (H', W') = size or (int(h scale), int(w scale)), W' even where out_fmt
        subsamples horizontally and H' where vertically (ValueError otherwise).  fmt, out_fmt, matrix, full_range, depth, out_depth, msb,
        out_msb, siting, out_siting, width and out: as `HAT.forward_yuv` takes them.  Equal, bit for bit, to yuv.yuv_to_planes ->
        `upscale` -> yuv.planes_to_yuv (yuv.packed_to_planes / planes_to_packed for a packed side).  A centre-sited planar output is
        stored by hat_lte_query_yuv and no fp32 image is written (with out= the call then allocates nothing after the first call of a
        shape); an output with a co-sited axis ('left' / 'topleft' on a subsampled axis) or a packed one is the plane query into the
        workspace, then hat_planes_to_yuv_sited / hat_planes_to_packed422."""
        if not isinstance(frame, torch.Tensor):
            raise TypeError(f"upscale_yuv needs a uint8 device tensor, got {type(frame).__name__}")
        if frame.dtype not in (torch.uint8, torch.uint16):
            raise TypeError(f"upscale_yuv needs a uint8 tensor (uint16 with depth 10, 12 or 16), got {frame.dtype}")
        from .. import ops, yuv
        out_fmt = fmt if out_fmt is None else out_fmt
        out_siting = siting if out_siting is None else out_siting
        out_depth = depth if out_depth is None else out_depth
        src = ops.FrameSide(fmt, depth=depth, msb=msb, siting=siting)   # (refuses what is no layout, depth or siting)
        dst_side = ops.FrameSide(out_fmt, depth=out_depth, msb=out_msb, siting=out_siting)
        to_rgb, from_rgb = yuv.csc(matrix, full_range, depth)[0], yuv.csc(matrix, full_range, out_depth)[1]
        if frame.dtype != src.dtype:
            raise TypeError(f"upscale_yuv: depth={depth} {fmt} needs a {str(src.dtype)[6:]} tensor, got {frame.dtype}")
        if frame.dim() == 2:
            frame = frame.unsqueeze(0)
        if frame.dim() != 3:
            raise RuntimeError(f"expected (1,rows,w) {fmt} frames, got {tuple(frame.shape)}")
        if frame.shape[0] != 1:
            raise RuntimeError(f"ESCLTE.upscale_yuv takes one frame per call, got a batch of {frame.shape[0]}")
        H, W = src.size(frame.shape, width)
        h, w = self._out_size("upscale_yuv", H, W, size, scale)
        odd = dst_side.size_refusal(h, w)
        if odd:
            raise ValueError(f"ESCLTE.upscale_yuv: an output of {h}x{w} is no {out_fmt} frame: the layout needs an even {odd}")
        self._check_call(frame)
        with torch.no_grad():
            eng = self.engine(frame.device)
            dst = dst_side.out(out, (1,) + dst_side.shape(h, w), eng.dev)
            eng.gen_feat_frame(H, W, lambda x: src.to_planes(frame, x, to_rgb, width=W))
            self._feat_engine = eng
            cells = self._cells(H, W, h, w, scale_max)
            if dst_side.fusable:
                eng.query_grid_yuv(dst_side.views(dst), cells, from_rgb, dst_side.sub, out_depth, dst_side.msb)
            else:   # the 2-tap filter of a co-sited axis needs a halo a 4 x 8 tile does not have; a packed unit spans tiles
                planes = eng.query_grid_planes(eng.planes_buffer(H, W, h, w), cells, out_affine=(0.5, 0.5))
                dst_side.from_planes(planes, dst, from_rgb, width=w)
            return dst
