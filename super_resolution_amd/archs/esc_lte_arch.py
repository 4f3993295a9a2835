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
    One frame per call.  `forward_ensemble`, the byte and YCbCr paths, row bands and plans raise NotImplementedError, as for `ESC`."""

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
