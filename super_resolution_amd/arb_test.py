"""The ESC-LTE benchmark loop, the reference's ESC/esc_arb/test.py (eval_psnr over the files of esc_arb/configs/test/) on the MI355X.

    python -m super_resolution_amd.arb_test --config test-set5-4.yaml --model ckpt.pth [--scale_max 4] [--fast ...] [--window 0]

`--config` is one of the reference's test configs, read unchanged: `test_dataset.dataset` of `paired-image-folders` with the wrapper
`sr-implicit-paired[-fast]` (LR and GT folders) or of `image-folder` with `sr-implicit-downsampled[-fast]` (a GT folder; the LR
image is Pillow's 8-bit bicubic resize of the GT, made on the device), `eval_type` (`benchmark-S`, `div2k-S` or none),
`eval_bsize` and `data_norm`.  `--model` is the reference's checkpoint (`ESCLTE.from_checkpoint`).  Every image is read as bytes
and uploaded as bytes; the LR frame, the network, the query at the ground truth's size and the score run on the device
(`ESCLTE.score_u8` / `score_gt_u8`) and one score per image comes back.  Prints the running mean per image and a
last line `result: {:.4f}`, as test.py does.

`eval_bsize` and `--fast` are accepted and change nothing: the whole grid is one fused query here, whose arithmetic does not
depend on how the reference would have batched it.  Refused, with a message: a `data_norm` other than sub 0.5 / div 0.5 (the
device path normalises with exactly that), `--window` other than 0 (ESC reflects its own window edges; the SwinIR padding branch is
not built), the training options `inp_size`, `augment` and `sample_q`, a `scale_max` of the downsampled wrapper that differs from
its `scale_min` (a random scale per image), `split_file` and `cache: bin`, and every other dataset or wrapper.
"""
from __future__ import annotations

import argparse
import math
import sys

MIN_LR_SIDE = 17   # ESC pads a frame to its 32-pixel window by reflection: the padding 32 - n must be smaller than the side n
PAIRED = ("sr-implicit-paired", "sr-implicit-paired-fast")
DOWNSAMPLED = ("sr-implicit-downsampled", "sr-implicit-downsampled-fast")


# ---- the arithmetic of the loop: no device, no files ----
def parse_eval_type(eval_type):
    """test.py:47-56 with utils.py:136, :142 -> (mode, shave, S): None -> (None, 0, None); 'benchmark-S' -> ('benchmark', S, S);
    'div2k-S' -> ('div2k', S + 6, S); anything else is a NotImplementedError, as in the reference."""
    if eval_type is None:
        return None, 0, None
    if isinstance(eval_type, str) and eval_type.startswith(("div2k", "benchmark")):
        mode = "div2k" if eval_type.startswith("div2k") else "benchmark"
        try:
            S = int(eval_type.split("-")[1])
        except (IndexError, ValueError):
            raise NotImplementedError(f"eval_type {eval_type!r}: expected 'benchmark-S' or 'div2k-S' with an integer S") from None
        if S < 0:
            raise NotImplementedError(f"eval_type {eval_type!r}: a negative scale")
        return mode, (S + 6 if mode == "div2k" else S), S
    raise NotImplementedError(f"eval_type {eval_type!r} is not built: the reference knows 'benchmark-S', 'div2k-S' and none")


def cell_factor(S, scale_max) -> float:
    """test.py:90-92: cell * max(scale / scale_max, 1), `scale` the integer of eval_type (NOT the image's own ratio); no eval_type
    leaves the cell as it is."""
    return 1.0 if S is None else max(S / scale_max, 1)


def eval_cells(h: int, w: int, S, scale_max):
    """The (cy, cx) of an (h, w) query grid: 2 / n rounded to fp32 (wrappers.py:70-72, :139), times cell_factor in fp32."""
    import torch
    f = cell_factor(S, scale_max)
    return tuple(float(torch.tensor(2 / n, dtype=torch.float32) * f) for n in (h, w))


def paired_sizes(h_lr: int, w_lr: int, H: int, W: int):
    """wrappers.py:30-34: s = H // h_lr; the ground truth is cropped to (h_lr s, w_lr s) -> (s, (h, w))."""
    h_lr, w_lr, H, W = int(h_lr), int(w_lr), int(H), int(W)
    if min(h_lr, w_lr, H, W) < 1:
        raise ValueError(f"an LR frame of {h_lr}x{w_lr} with a ground truth of {H}x{W}: an empty side")
    s = H // h_lr
    if s < 1 or w_lr * s > W:
        raise ValueError(f"an LR frame of {h_lr}x{w_lr} and a ground truth of {H}x{W} are no pair: the scale H // h = {s} needs a ground "
                         f"truth of at least {h_lr * max(s, 1)}x{w_lr * max(s, 1)}")
    return s, (h_lr * s, w_lr * s)


def downsampled_sizes(H: int, W: int, scale):
    """wrappers.py:176-180: per axis n_lr = floor(N / scale + 1e-9), the ground truth cropped to round(n_lr scale) (Python's round)
    -> ((h_lr, w_lr), (h, w))."""
    if not scale >= 1:
        raise ValueError(f"a scale of {scale} does not shrink the ground truth")
    lr = tuple(math.floor(int(n) / scale + 1e-9) for n in (H, W))
    if min(lr) < 1:
        raise ValueError(f"a {H}x{W} ground truth cannot be shrunk by {scale}")
    return lr, tuple(round(n * scale) for n in lr)


def check_lr_size(h_lr: int, w_lr: int):
    if min(h_lr, w_lr) < MIN_LR_SIDE:
        raise ValueError(f"an LR frame of {h_lr}x{w_lr} is too small: ESC's 32-pixel window is filled by reflection, which needs sides of "
                         f"at least {MIN_LR_SIDE}")


def psnr_of(total: float, terms: int) -> float:
    return float("inf") if total == 0 else -10.0 * math.log10(total / terms)


# ---- the config ----
def _is_half(v) -> bool:
    v = v if isinstance(v, (list, tuple)) else [v]
    return len(v) >= 1 and all(float(x) == 0.5 for x in v)


def parse_config(config: dict) -> dict:
    """One of the reference's test configs -> {kind: 'paired' | 'downsampled', roots: (lr, gt) | (gt,), scale, first_k, repeat,
    eval_type, eval_bsize}; refusals as the module's docstring lists them."""
    spec = config.get("test_dataset")
    if not isinstance(spec, dict) or "dataset" not in spec or "wrapper" not in spec:
        raise ValueError("the config needs test_dataset.dataset and test_dataset.wrapper")
    ds, wr = spec["dataset"], spec["wrapper"]
    dargs, wargs = dict(ds.get("args") or {}), dict(wr.get("args") or {})
    parse_eval_type(config.get("eval_type"))
    norm = config.get("data_norm") or {}
    for side in ("inp", "gt"):
        t = norm.get(side) or {}
        if not (_is_half(t.get("sub", [0])) and _is_half(t.get("div", [1]))):
            raise NotImplementedError(f"data_norm.{side} = {t or None}: only sub 0.5 / div 0.5 is built (the device path normalises with it)")
    for key in ("inp_size", "augment", "sample_q"):
        if wargs.get(key):
            raise NotImplementedError(f"wrapper option {key} = {wargs[key]!r} is a training option: the benchmark loop scores whole images")
    if dargs.get("split_file") is not None:
        raise NotImplementedError("dataset option split_file is not built: the folder's sorted images are the set")
    if dargs.get("cache", "none") not in ("none", "in_memory"):
        raise NotImplementedError(f"dataset option cache = {dargs['cache']!r} is not built (it only changes how the reference loads files)")
    out = dict(first_k=dargs.get("first_k"), repeat=int(dargs.get("repeat", 1)), eval_type=config.get("eval_type"),
               eval_bsize=config.get("eval_bsize"), scale=None)
    if wr.get("name") in PAIRED:
        if ds.get("name") != "paired-image-folders":
            raise ValueError(f"wrapper {wr.get('name')} needs a paired-image-folders dataset, got {ds.get('name')!r}")
        return dict(out, kind="paired", roots=(dargs["root_path_1"], dargs["root_path_2"]))
    if wr.get("name") in DOWNSAMPLED:
        if ds.get("name") != "image-folder":
            raise ValueError(f"wrapper {wr.get('name')} needs an image-folder dataset, got {ds.get('name')!r}")
        smin = wargs.get("scale_min", 1)
        smax = wargs.get("scale_max")
        if smax is not None and smax != smin:
            raise NotImplementedError(f"wrapper scale_min {smin} / scale_max {smax}: a random scale per image is a training option")
        return dict(out, kind="downsampled", roots=(dargs["root_path"],), scale=smin)
    raise NotImplementedError(f"wrapper {wr.get('name')!r} is not built: only {', '.join(PAIRED + DOWNSAMPLED)} (DESIGN.md §7)")


def list_items(cfg: dict):
    """The image paths of the set, one tuple per item, in the reference's order (sorted names, first_k, repeat)."""
    from .data import _scan
    cols = []
    for root in cfg["roots"]:
        files = _scan(root)
        cols.append(files if cfg["first_k"] is None else files[:int(cfg["first_k"])])
    if len({len(c) for c in cols}) != 1:
        raise ValueError(f"the folders {cfg['roots']} hold different numbers of images: {[len(c) for c in cols]}")
    return list(zip(*cols)) * cfg["repeat"]


def read_u8(path: str):
    """An image file as (h,w,3) uint8 RGB bytes (PIL, as data.read_image opens it; no division)."""
    import numpy as np
    import torch
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m super_resolution_amd.arb_test", description=__doc__.split("\n\n")[0],
                                 epilog="eval_bsize (config) and --fast are accepted and do not change the arithmetic: the whole grid is one "
                                        "fused query on the device.  --window other than 0 is refused: ESC reflects its own window edges.")
    ap.add_argument("--config", required=True, help="one of the reference's esc_arb/configs/test files")
    ap.add_argument("--model", required=True, help="the reference's checkpoint: {'model': {'name': 'lte', 'args': ..., 'sd': ...}}")
    ap.add_argument("--window", default="0", help="only 0: ESC reflects its own window edges")
    ap.add_argument("--scale_max", "--scale-max", dest="scale_max", default="4", help="the largest trained scale: the cell is clipped above it")
    ap.add_argument("--fast", nargs="?", const=True, default=False, help="accepted; the query is one fused launch either way")
    ap.add_argument("--gpu", default="0")
    ap.add_argument("--compute-dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if int(args.window) != 0:
        ap.error("--window other than 0 is not built: ESC reflects its own window edges, the SwinIR padding branch does not apply")
    import torch
    import yaml
    with open(args.config, "r") as f:
        cfg = parse_config(yaml.safe_load(f))
    items = list_items(cfg)
    if not torch.cuda.is_available():
        raise RuntimeError("super_resolution_amd.arb_test needs a GPU: the MI355X HIP path is the only path (no CPU fallback)")
    from .archs.esc_lte_arch import ESCLTE
    dev = torch.device("cuda", int(args.gpu))
    net = ESCLTE.from_checkpoint(torch.load(args.model, map_location="cpu", weights_only=True), compute_dtype=args.compute_dtype).to(dev)
    scale_max, total = int(args.scale_max), 0.0
    for n, paths in enumerate(items, 1):
        frames = [read_u8(p).to(dev) for p in paths]
        if cfg["kind"] == "paired":
            res = net.score_u8(frames[0], frames[1], eval_type=cfg["eval_type"], scale_max=scale_max)
        else:
            res = net.score_gt_u8(frames[0], cfg["scale"], eval_type=cfg["eval_type"], scale_max=scale_max)
        total += res
        print("val {:.4f}".format(total / n), flush=True)
    print("result: {:.4f}".format(total / max(len(items), 1)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
