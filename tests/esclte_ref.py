"""A torch restatement of ESC-LTE (the reference's ESC/esc_arb: models/lte.py:23-109 over models/esc.py:255-296, inference.py:51-74)
from its state dict, for the tests of the device path: the goldens under tests/golden/esclte_*.npz come from the reference itself
(gen_golden_esclte.py).  Plain torch on the CPU in the reference's operation order, in the dtype of the state dict: pass `d64(sd)`
and double inputs for the fp64 restatement.  The encoder is tests/esc_ref.py's."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import esc_ref
from esc_ref import GOLDEN, W_SEED, X_SEED, d64, template_from_surface  # noqa: F401
from super_resolution_amd import synth

HIDDEN = 256
ENC = dict(esc_ref.BASE, exp_ratio=1.25)
FRAME = (1, 3, 20, 24)
N_SCATTER = 143
LAST_SCALE = 1.0   # the generator's factor on imnet.layers.6 (1: the seeded weights already give an output of O(1))
CASES = {   # name -> (encoder keywords, frame, what is queried)
    "a": (dict(ENC, n_blocks=1, conv_blocks=1), FRAME, dict(grid=(30, 41), scale_max=4)),     # x1.5 / x1.708: unequal axes
    "b": (dict(ENC, n_blocks=1, conv_blocks=1), FRAME, dict(grid=(20, 24), scale_max=4)),     # x1: every rel is 0 or +-2
    "c": (dict(ENC, n_blocks=1, conv_blocks=1), FRAME, dict(grid=(100, 120), scale_max=4)),   # x5: the cell is clipped at scale_max
    "d": (dict(ENC, n_blocks=2, conv_blocks=1), FRAME, dict(scatter=N_SCATTER)),              # scattered, with -1 and 1 on both axes
}


def make_coord(shape, dtype=torch.float32):
    """esc_arb/utils.py:105-120 (flatten=True): pixel centres in [-1, 1], (y, x) order, computed in fp32 as the reference does."""
    seqs = []
    for n in shape:
        r = 2 / (2 * n)
        seqs.append(-1 + r + (2 * r) * torch.arange(n).float())
    return torch.stack(torch.meshgrid(*seqs, indexing="ij"), dim=-1).view(-1, len(shape)).to(dtype)


def grid_cell(hw, HW, scale_max=4):
    """inference.py:64-70: the cell of every query of an (h, w) grid over an (H, W) frame -> (cell_y, cell_x) as fp32 tensors."""
    factor = max((hw[0] / HW[0]) / scale_max, 1)
    return tuple(factor * (torch.ones(1) * (2 / n)) for n in hw)


def grid_queries(hw, HW, scale_max=4):
    coord = make_coord(hw)
    cy, cx = grid_cell(hw, HW, scale_max)
    return coord, torch.stack([cy.expand(coord.shape[0]), cx.expand(coord.shape[0])], dim=-1).contiguous()


def scatter_queries(key: str, n: int = N_SCATTER, scale: float = 2.7, HW=FRAME[2:]):
    """n seeded coordinates in [-1, 1] whose first eight put exactly -1 and 1 on both axes; cells of a x`scale` grid, jittered."""
    coord = synth.uniform(X_SEED, key + ".coord", (n, 2)) * 2 - 1
    edge = torch.tensor([[-1, -1], [-1, 1], [1, -1], [1, 1], [-1, 0.3], [1, -0.2], [0.1, -1], [-0.7, 1]], dtype=torch.float32)
    m = min(n, len(edge))
    coord[:m] = edge[:m]
    cell = torch.tensor([2 / (HW[0] * scale), 2 / (HW[1] * scale)], dtype=torch.float32) * (0.5 + synth.uniform(X_SEED, key + ".cell", (n, 2)))
    return coord.contiguous(), cell.contiguous()


def case_queries(name: str):
    _, frame, what = CASES[name]
    if "grid" in what:
        return grid_queries(what["grid"], frame[2:], what["scale_max"])
    return scatter_queries("esclte_" + name, what["scatter"], HW=frame[2:])


def head_state_dict(seed: int = W_SEED, last_scale: float = LAST_SCALE) -> dict:
    """The head's parameters alone (kernel-level tests), seeded like the whole model's."""
    t = {"coef.weight": (HIDDEN, 64, 3, 3), "coef.bias": (HIDDEN,), "freq.weight": (HIDDEN, 64, 3, 3), "freq.bias": (HIDDEN,),
         "phase.weight": (HIDDEN // 2, 2)}
    for i in (0, 2, 4):
        t[f"imnet.layers.{i}.weight"], t[f"imnet.layers.{i}.bias"] = (HIDDEN, HIDDEN), (HIDDEN,)
    t["imnet.layers.6.weight"], t["imnet.layers.6.bias"] = (3, HIDDEN), (3,)
    return lte_state_dict({k: torch.zeros(v) for k, v in t.items()}, seed, last_scale)


def lte_state_dict(template: dict, seed: int = W_SEED, last_scale: float = LAST_SCALE) -> dict:
    """esc_ref.esc_state_dict over the reference LTE's surface, with the last imnet layer scaled by `last_scale`."""
    sd = esc_ref.esc_state_dict(template, seed)
    for k in ("imnet.layers.6.weight", "imnet.layers.6.bias"):
        sd[k] = sd[k] * last_scale
    return sd


def encoder(sd, cfg, x):
    """esc.py:287-296: ESC's forward without to_img, on the keys under `encoder.`."""
    enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    ws, heads, pdim = cfg["window_size"], cfg["num_heads"], cfg["pdim"]
    lk = esc_ref.geo_ensemble(enc["plk_filter"])
    feat = F.conv2d(x, enc["proj.weight"], enc["proj.bias"], padding=1)
    feat0 = feat
    for i in range(cfg["n_blocks"]):
        p, skip = f"blocks.{i}", feat
        t = esc_ref.convffn(esc_ref.layernorm(feat, enc[p + ".ln_proj.weight"], enc[p + ".ln_proj.bias"]), enc, p + ".proj")
        t = t + esc_ref.window_attention(esc_ref.layernorm(t, enc[p + ".ln_attn.weight"], enc[p + ".ln_attn.bias"]), enc, p + ".attn", ws, heads)
        for j in range(cfg["conv_blocks"]):
            z = esc_ref.plk(esc_ref.convffn(t, enc, f"{p}.convffns.{j}"), enc, f"{p}.pconvs.{j}", lk, pdim)
            t = t + F.conv2d(z, enc[f"{p}.pconvs.{j}.aggr.weight"], enc[f"{p}.pconvs.{j}.aggr.bias"])
        feat = F.conv2d(esc_ref.layernorm(t, enc[p + ".ln_out.weight"], enc[p + ".ln_out.bias"]), enc[p + ".conv_out.weight"],
                        enc[p + ".conv_out.bias"], padding=1) + skip
    return F.conv2d(feat, enc["last.weight"], enc["last.bias"], padding=1) + feat0


def coef_freq(sd, feat):
    """lte.py:30-31 -> (coef, freq), each (1,256,H,W)."""
    return (F.conv2d(feat, sd["coef.weight"], sd["coef.bias"], padding=1), F.conv2d(feat, sd["freq.weight"], sd["freq.bias"], padding=1))


def imnet(sd, x, act_round=None):
    """act_round: applied to the input and to the output of the first two hidden layers, the three places where hat_lte_query
    stores activations as T (the last hidden layer feeds the 256 -> 3 layer from the fp32 accumulators)."""
    rd = act_round or (lambda t: t)
    x = rd(x)
    for i in (0, 2, 4):
        x = F.relu(F.linear(x, sd[f"imnet.layers.{i}.weight"], sd[f"imnet.layers.{i}.bias"]))
        x = rd(x) if i != 4 else x
    return F.linear(x, sd["imnet.layers.6.weight"], sd["imnet.layers.6.bias"])


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def mfma_weights_as_bf16(sd):
    """The head's parameters with the three 256 x 256 layers (hat_lte_query's MFMA operands) rounded to bf16; everything else as is."""
    return {k: (bf16_round(v) if k in ("imnet.layers.0.weight", "imnet.layers.2.weight", "imnet.layers.4.weight") else v) for k, v in sd.items()}


def without_hidden_group(sd, g):
    """The head with channels 16 g .. 16 g + 15 of the last hidden layer dropped: their columns of the 256 -> 3 layer are zero."""
    sd = dict(sd)
    w = sd["imnet.layers.6.weight"].clone()
    w[:, 16 * g: 16 * g + 16] = 0
    sd["imnet.layers.6.weight"] = w
    return sd


def bilinear_base(inp, coord):
    """The bilinear base image of the head (lte.py:102-104) by explicit indexing, in fp64: inp (1,3,H,W), coord (1,Q,2) as (y, x) in
    [-1, 1], align_corners=False, border padding -> (1,Q,3)."""
    H, W = inp.shape[-2:]
    m, c = inp[0].double(), coord[0].double()
    iy, ix = (((c[:, 0] + 1) * H - 1) / 2).clamp(0, H - 1), (((c[:, 1] + 1) * W - 1) / 2).clamp(0, W - 1)
    y0, x0 = iy.floor().long(), ix.floor().long()
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    ty, tx = iy - y0, ix - x0
    v = m[:, y0, x0] * (1 - tx) * (1 - ty) + m[:, y0, x1] * tx * (1 - ty) + m[:, y1, x0] * (1 - tx) * ty + m[:, y1, x1] * tx * ty
    return v.t()[None]


def head(sd, coef, freq, inp, coord, cell, act_round=None):
    """lte.py:34-105, statement for statement.  coef, freq (1,256,H,W); inp (1,3,H,W); coord, cell (1,Q,2) -> (1,Q,3).
    act_round: see imnet (None: the reference)."""
    dt = coef.dtype
    coord, cell = coord.to(dt), cell.to(dt)
    H, W = coef.shape[-2:]
    rx, ry = 2 / H / 2, 2 / W / 2   # (the reference's names: "x" is axis 0)
    feat_coord = make_coord((H, W), dt).view(H, W, 2).permute(2, 0, 1).unsqueeze(0)
    near = lambda t, c: F.grid_sample(t, c.flip(-1).unsqueeze(1), mode="nearest", align_corners=False)[:, :, 0, :].permute(0, 2, 1)
    preds, areas = [], []
    for vx in (-1, 1):
        for vy in (-1, 1):
            coord_ = coord.clone()
            coord_[:, :, 0] += vx * rx + 1e-6
            coord_[:, :, 1] += vy * ry + 1e-6
            coord_.clamp_(-1 + 1e-6, 1 - 1e-6)
            q_coef, q_freq, q_coord = near(coef, coord_), near(freq, coord_), near(feat_coord, coord_)
            rel = coord - q_coord
            rel[:, :, 0] *= H
            rel[:, :, 1] *= W
            rel_cell = cell.clone()
            rel_cell[:, :, 0] *= H
            rel_cell[:, :, 1] *= W
            bs, q = coord.shape[:2]
            q_freq = torch.stack(torch.split(q_freq, 2, dim=-1), dim=-1)
            q_freq = torch.sum(torch.mul(q_freq, rel.unsqueeze(-1)), dim=-2)
            q_freq = q_freq + F.linear(rel_cell.view(bs * q, -1), sd["phase.weight"]).view(bs, q, -1)
            q_freq = torch.cat((torch.cos(math.pi * q_freq), torch.sin(math.pi * q_freq)), dim=-1)
            preds.append(imnet(sd, torch.mul(q_coef, q_freq).contiguous().view(bs * q, -1), act_round).view(bs, q, -1))
            areas.append(torch.abs(rel[:, :, 0] * rel[:, :, 1]) + 1e-9)
    tot = torch.stack(areas).sum(dim=0)
    areas = areas[::-1]   # the diagonal swap (lte.py:96-97)
    ret = 0
    for pred, area in zip(preds, areas):
        ret = ret + pred * (area / tot).unsqueeze(-1)
    return ret + F.grid_sample(inp, coord.flip(-1).unsqueeze(1), mode="bilinear", padding_mode="border",
                               align_corners=False)[:, :, 0, :].permute(0, 2, 1)


def forward(sd, cfg, inp, coord, cell):
    """model(inp, coord, cell) (lte.py:107-109) in the dtype of sd / inp: inp (1,3,H,W) normalised, coord / cell (1,Q,2) -> (1,Q,3)."""
    coef, freq = coef_freq(sd, encoder(sd, cfg, inp))
    return head(sd, coef, freq, inp, coord, cell)


def upscale(sd, cfg, img, hw, scale_max=4):
    """inference.py:64-73 without the clamp: img (1,3,H,W) in [0, 1] -> (1,3,h,w)."""
    coord, cell = grid_queries(hw, img.shape[-2:], scale_max)
    y = forward(sd, cfg, (img - 0.5) / 0.5, coord[None].to(img.dtype), cell[None].to(img.dtype))
    return (y * 0.5 + 0.5).view(hw[0], hw[1], 3).permute(2, 0, 1)[None]


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def surfaces() -> dict:
    with open(os.path.join(GOLDEN, "esclte_surface.json")) as f:
        return json.load(f)


def load_case(name: str):
    """-> (encoder cfg, state dict regenerated from the seed, golden arrays x / coord / cell / y, meta) of whole-model case a..d."""
    meta = surfaces()
    g = dict(np.load(os.path.join(GOLDEN, f"esclte_{name}.npz")))
    m = meta["cases"][name]
    sd = lte_state_dict(template_from_surface(m["surface"]), meta["w_seed"], meta["last_scale"])
    return m["cfg"], sd, g, m
