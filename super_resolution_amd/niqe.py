"""NIQE (Natural Image Quality Evaluator): the DEFINITION, on the host, of what csrc/hat_niqe.hip sums.

This is the no-reference score of the reference's GT-less test sets (basicsr/metrics/niqe.py, `calculate_niqe`; used by
options/test/HAT_GAN_Real_SRx4.yml's kind of run).  numpy only: no scipy, no OpenCV.  The steps and their dtypes are the
reference's, one by one, because the reference runs in float32 and its result depends on that:

  y_plane      float32 image on [0, 255] -> BT.601 Y (metrics.to_y_channel: fp64 dot product, float32(y / 255) * 255) -> crop
               the border -> round half to even -> crop to whole 96 x 96 blocks (niqe.py:182-195, :100-103).
  mscn         mu = conv7x7(img), sigma = sqrt(|conv7x7(img^2) - mu^2|), n = (img - mu) / (sigma + 1) with `nearest` borders
               (niqe.py:107-110).  scipy.ndimage.convolve of a float32 image accumulates the 49 taps in a double, in raster
               order, product and sum rounded one by one, and ROUNDS THE RESULT TO FLOAT32; img^2, mu^2, the subtraction
               (values up to 65025, ulp 0.004: a float32 cancellation), the root and the quotient are float32 operations.
               On smooth regions sigma is visibly not what an fp64 evaluation gives; the thing to match is the reference.
  block_stats  per block (96 x 96, at the second scale 48 x 48) and per map -- n and n * roll(n, s) for s = (0,1), (1,0),
               (1,1), (1,-1), np.roll wrapping INSIDE the block (niqe.py:58-61) -- the five numbers an AGGD fit needs: the
               count of negative values, the count of positive values, the sum of squares (each square a float32) over the
               negative values, over the positive values, and the sum of absolute values.  25 numbers per block and scale,
               index 5 * map + quantity.  `acc=np.float32` adds them as the reference does (numpy's pairwise float32 sum
               over the raster-ordered values), `acc=np.float64` adds the same float32 values in fp64: what the device does.
  features_from_stats  the AGGD fits (niqe.py:13-65) from those numbers in the reference's float32 scalar arithmetic, alpha by
               argmin on the 9801-point grid in fp64.  A block without negative or without positive values gives NaN where
               the reference gives NaN -- and alpha = 0.2 there, as the reference's argmin over NaNs returns position 0.
  score        nanmean / cov over the complete rows / pinv, fp64 (niqe.py:126-141).  No complete row -> NaN.

The second scale is resize.imresize(img / 255, 0.5) * 255 (niqe.py:122-124).  The 7 x 7 window is computed:
exp(-(x^2 + y^2) / (2 (7/6)^2)) over its sum equals the `gaussian_window` of the reference's parameter file to 1.4e-17.

The pristine model (mu_pris_param: 36 doubles, cov_pris_param: 36 x 36) is data of the reference and is not part of this
package.  pris_params() takes it from, in this order: the `pris_params` argument (a path to an .npz or a dict; the YAML
metric entry's `pris_params:` key), the environment variable HAT_NIQE_PRIS_PARAMS, niqe_pris_params.npz beside an installed
basicsr.metrics (located with importlib.util.find_spec; nothing is imported).  None of them -> RuntimeError.
"""
from __future__ import annotations

import importlib.util
import math
import os

import numpy as np

from . import resize
from .metrics import to_y_channel

_F = np.float32
BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))   # np.roll(block, s, axis=(0, 1)) of maps 1..4; map 0 is n itself
ENV_PRIS = "HAT_NIQE_PRIS_PARAMS"
PRIS_FILE = "niqe_pris_params.npz"


def gaussian_window() -> np.ndarray:
    """The 7 x 7 window, float64, symmetric: exp(-(x^2 + y^2) / (2 (7/6)^2)) / sum."""
    x = np.arange(7, dtype=np.float64) - 3.0
    g = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


_grid = None


def _aggd_grid():
    """gam = arange(0.2, 10.001, 0.001) and r_gam = gamma(2/g)^2 / (gamma(1/g) gamma(3/g)) (niqe.py:24-26), computed once."""
    global _grid
    if _grid is None:
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        g1 = np.array([math.gamma(v) for v in rec])
        g2 = np.array([math.gamma(v) for v in rec * 2])
        g3 = np.array([math.gamma(v) for v in rec * 3])
        _grid = (gam, np.square(g2) / (g1 * g3))
    return _grid


def y_plane(img_u8: np.ndarray, crop_border: int, bgr: bool = False) -> np.ndarray:
    """(h,w,3) image with values on [0, 255] -> the rounded, block-cropped float32 Y plane the two scales start from."""
    img = np.asarray(img_u8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"y_plane takes an (h,w,3) image, got {img.shape}")
    if bgr:
        img = img[:, :, ::-1]
    return _prepare(to_y_channel(img.astype(_F))[..., 0], crop_border)


def _prepare(plane: np.ndarray, crop_border: int) -> np.ndarray:
    crop_border = int(crop_border)
    if crop_border != 0:
        plane = plane[crop_border:-crop_border, crop_border:-crop_border]
    plane = np.round(plane.astype(_F))
    nbh, nbw = plane.shape[0] // BLOCK, plane.shape[1] // BLOCK
    if nbh < 1 or nbw < 1:
        raise ValueError(f"NIQE needs at least one {BLOCK}x{BLOCK} block after cropping, got {plane.shape[0]}x{plane.shape[1]}")
    return np.ascontiguousarray(plane[:nbh * BLOCK, :nbw * BLOCK])


def _conv7(img: np.ndarray, win: np.ndarray) -> np.ndarray:
    """scipy.ndimage.convolve(img, win, mode='nearest') of a float32 image: 49 taps in a double in raster order, rounded to
    float32 at the end."""
    h, w = img.shape
    p = np.pad(img, 3, mode="edge").astype(np.float64)
    wf = win[::-1, ::-1]   # a convolution correlates with the flipped window (the window is symmetric)
    acc = np.zeros((h, w), dtype=np.float64)
    for a in range(7):
        for b in range(7):
            acc = acc + wf[a, b] * p[a:a + h, b:b + w]
    return acc.astype(_F)


def mscn(plane: np.ndarray) -> np.ndarray:
    """float32 (h,w) -> the float32 locally normalised plane n (niqe.py:107-110)."""
    img = np.asarray(plane)
    if img.dtype != _F or img.ndim != 2:
        raise ValueError(f"mscn takes a float32 (h,w) plane, got {img.shape} {img.dtype}")
    win = gaussian_window()
    mu = _conv7(img, win)
    sigma = np.sqrt(np.abs(_conv7(np.square(img), win) - np.square(mu)))
    return (img - mu) / (sigma + _F(1.0))


def block_maps(blk: np.ndarray):
    """The five float32 maps of one block: n, then n * roll(n, s) for s in SHIFTS."""
    return [blk] + [blk * np.roll(blk, s, axis=(0, 1)) for s in SHIFTS]


def block_stats(n: np.ndarray, block: int, acc=np.float32) -> np.ndarray:
    """float32 (h,w) with h, w multiples of `block` -> float64 (h / block, w / block, 25); acc: the type the sums are added in."""
    n = np.asarray(n)
    if n.dtype != _F or n.ndim != 2 or n.shape[0] % block or n.shape[1] % block or min(n.shape) < block:
        raise ValueError(f"block_stats takes a float32 plane of whole {block}x{block} blocks, got {n.shape} {n.dtype}")
    nbh, nbw = n.shape[0] // block, n.shape[1] // block
    out = np.zeros((nbh, nbw, 25), dtype=np.float64)
    for i in range(nbh):
        for j in range(nbw):
            blk = n[i * block:(i + 1) * block, j * block:(j + 1) * block]
            for m, v in enumerate(block_maps(blk)):
                v = v.flatten()
                neg, pos = v[v < 0], v[v > 0]
                out[i, j, 5 * m:5 * m + 5] = (neg.size, pos.size, np.sum(neg ** 2, dtype=acc), np.sum(pos ** 2, dtype=acc),
                                              np.sum(np.abs(v), dtype=acc))
    return out


def features_from_stats(stats: np.ndarray, block: int = BLOCK) -> np.ndarray:
    """(nbh, nbw, 25) sums of block x block blocks -> (nbh * nbw, 18) features, rows in the reference's order (block columns
    outermost).  The sums are rounded to float32 and the fit follows estimate_aggd_param / compute_feature in their dtypes.
    `block` gives the number of values per map (the counts leave out the zeros): 96, and 48 for the second scale."""
    s = np.asarray(stats, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 25:
        raise ValueError(f"features_from_stats takes (nbh, nbw, 25) sums, got {s.shape}")
    s = s.transpose(1, 0, 2).reshape(-1, 5, 5)
    nblk, npix = s.shape[0], _F(int(block) * int(block))
    gam, r_gam = _aggd_grid()
    feat = np.empty((nblk, 18), dtype=np.float64)
    with np.errstate(all="ignore"):
        for m in range(5):
            cn, cp = s[:, m, 0].astype(_F), s[:, m, 1].astype(_F)
            sn, sp, sa = s[:, m, 2].astype(_F), s[:, m, 3].astype(_F), s[:, m, 4].astype(_F)
            left, right = np.sqrt(sn / cn), np.sqrt(sp / cp)
            gammahat = left / right
            rhat = np.square(sa / npix) / ((sn + sp) / npix)
            rhatnorm = (rhat * (np.power(gammahat, 3) + _F(1)) * (gammahat + _F(1))) / np.square(np.square(gammahat) + _F(1))
            alpha = np.empty(nblk, dtype=np.float64)
            for k0 in range(0, nblk, 256):   # argmin over the grid, 256 blocks at a time; an all-NaN row gives position 0
                d = (r_gam[None, :] - rhatnorm[k0:k0 + 256, None].astype(np.float64)) ** 2
                alpha[k0:k0 + 256] = gam[np.argmin(d, axis=1)]
            ratio = np.sqrt(np.array([math.gamma(1 / a) / math.gamma(3 / a) for a in alpha]))
            beta_l, beta_r = left.astype(np.float64) * ratio, right.astype(np.float64) * ratio
            if m == 0:
                feat[:, 0], feat[:, 1] = alpha, (beta_l + beta_r) / 2
            else:
                mean = (beta_r - beta_l) * np.array([math.gamma(2 / a) / math.gamma(1 / a) for a in alpha])
                feat[:, 4 * m - 2:4 * m + 2] = np.stack([alpha, mean, beta_l, beta_r], axis=1)
    return feat


def score(feat1: np.ndarray, feat2: np.ndarray, pris) -> float:
    """The two scales' (nblocks, 18) features + the pristine model -> the NIQE score (niqe.py:126-141).  NaN when no block has
    all 36 features (an all-flat image): the reference's covariance of no rows is NaN as well."""
    mu_p, cov_p = pris_params(pris)
    dist = np.concatenate([np.asarray(feat1, np.float64), np.asarray(feat2, np.float64)], axis=1)
    complete = dist[~np.isnan(dist).any(axis=1)]
    if complete.shape[0] < 2:
        return float("nan")
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mu_d = np.nanmean(dist, axis=0)
    if np.isnan(mu_d).any():
        return float("nan")
    cov_d = np.cov(complete, rowvar=False)
    inv = np.linalg.pinv((cov_p + cov_d) / 2)
    d = (mu_p - mu_d).reshape(1, -1)
    return float(np.squeeze(np.sqrt(np.matmul(np.matmul(d, inv), d.T))))


def pris_params(source=None):
    """(mu_pris_param float64 (36,), cov_pris_param float64 (36,36)) from `source` (a dict, an .npz path, or an already loaded
    pair), else $HAT_NIQE_PRIS_PARAMS, else niqe_pris_params.npz beside an installed basicsr.metrics."""
    if isinstance(source, tuple) and len(source) == 2:
        return source
    tried = []
    if source is None:
        env = os.environ.get(ENV_PRIS)
        if env:
            source = env
        else:
            tried.append(f"${ENV_PRIS} is not set")
            try:
                spec = importlib.util.find_spec("basicsr")
            except (ImportError, ValueError):
                spec = None
            for root in (spec.submodule_search_locations if spec is not None and spec.submodule_search_locations else []):
                cand = os.path.join(root, "metrics", PRIS_FILE)
                if os.path.exists(cand):
                    source = cand
                    break
            if source is None:
                tried.append(f"no installed basicsr package holds metrics/{PRIS_FILE}")
    if source is None:
        raise RuntimeError("NIQE needs the pristine model (mu_pris_param, cov_pris_param), which is data of the reference and not part "
                           f"of this package: pass `pris_params` (a path to {PRIS_FILE} or a dict; in a YAML, the metric entry's "
                           f"`pris_params:` key) or set ${ENV_PRIS}.  Tried: {'; '.join(tried)}")
    if isinstance(source, (str, os.PathLike)):
        if not os.path.exists(source):
            raise RuntimeError(f"NIQE pristine model: {os.fspath(source)!r} does not exist")
        with np.load(source) as z:
            source = {k: z[k] for k in z.files}
    try:
        mu = np.asarray(source["mu_pris_param"], dtype=np.float64).reshape(-1)
        cov = np.asarray(source["cov_pris_param"], dtype=np.float64)
    except (KeyError, TypeError, IndexError) as e:
        raise RuntimeError("NIQE pristine model: need the entries mu_pris_param (36) and cov_pris_param (36 x 36)") from e
    if mu.shape != (36,) or cov.shape != (36, 36):
        raise RuntimeError(f"NIQE pristine model: mu_pris_param {mu.shape} / cov_pris_param {cov.shape} are not (36,) / (36, 36)")
    return mu, cov


def half_plane(plane: np.ndarray) -> np.ndarray:
    """The second scale's image: imresize(plane / 255, 0.5, antialiasing) * 255, float32 (niqe.py:122-124)."""
    return resize.imresize((plane / _F(255.0))[None], 0.5, True)[0] * _F(255.0)


def stats_of(plane: np.ndarray, acc=np.float32):
    """The rounded, block-cropped Y plane -> (stats96, stats48): what ops.niqe_stats returns from the device."""
    return block_stats(mscn(plane), BLOCK, acc), block_stats(mscn(half_plane(plane)), BLOCK // 2, acc)


def niqe_of_plane(plane: np.ndarray, pris=None, acc=np.float32) -> float:
    pris = pris_params(pris)
    s1, s2 = stats_of(plane, acc)
    return score(features_from_stats(s1, BLOCK), features_from_stats(s2, BLOCK // 2), pris)


def calculate_niqe(img, crop_border, input_order="HWC", convert_to="y", pris_params=None, bgr=False, **_):
    """basicsr.metrics.calculate_niqe for RGB arrays (bgr=True: B, G, R bytes).  img: [0, 255], 'HWC', 'CHW' or 'HW'."""
    if input_order not in ("HWC", "CHW", "HW"):
        raise ValueError(f"Wrong input_order {input_order}. Supported input_orders are 'HWC', 'CHW' and 'HW'")
    img = np.asarray(img).astype(_F)
    if input_order == "HW":
        if img.ndim != 2:
            raise ValueError(f"input_order 'HW' takes an (h,w) plane, got {img.shape}")
        plane = _prepare(img, crop_border)
    else:
        if convert_to == "gray":
            raise NotImplementedError("calculate_niqe: convert_to 'gray' is cv2.cvtColor's BGR2GRAY in the reference, whose float "
                                      "arithmetic cannot be pinned without OpenCV; use convert_to 'y'")
        if convert_to != "y":
            raise ValueError(f"calculate_niqe: convert_to is 'y' (or 'gray', unsupported), got {convert_to!r}")
        if input_order == "CHW":
            img = img.transpose(1, 2, 0)
        plane = y_plane(img, crop_border, bgr=bgr)
    return niqe_of_plane(plane, pris_params)
