"""super_resolution_amd/resize.py, the host definition of the MATLAB-style bicubic imresize, against golden vectors of the
reference's `imresize` / `calculate_weights_indices` (tests/golden/gen_golden_resize.py); the GT-only dataset built on it; the
C prototypes of the device entries.  The tables must equal the reference's bit for bit.  The pixels cannot (the reference sums
with Tensor.mv, whose order is unspecified), so they are held to the bound derived from the tables themselves:
(P_h S_h + P_w S_w S_h) 2^-24 max|img|, S = max_i sum_k |w[i,k]| — every output is a sum of P products of values bounded by
max|img| (S_h max|img| after the H pass), and two fp32 evaluations of such a sum differ by at most P sum|w| max|v| 2^-24 to
first order."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import golden
from super_resolution_amd import resize as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = golden("imresize.npz")
CASES = json.loads(str(G["cases"]))
WANT = [("x4", 48, 68, 1 / 4, True), ("x3", 48, 66, 1 / 3, True), ("x2", 50, 70, 1 / 2, True), ("s075", 37, 53, 0.75, True),
        ("s03", 50, 70, 0.3, True), ("up2", 20, 28, 2.0, True), ("up3", 19, 23, 3.0, True), ("tiny", 9, 9, 1 / 4, True),
        ("x2_noaa", 50, 70, 1 / 2, False)]


def test_the_golden_file_holds_the_cases():
    assert [(c["name"], c["h"], c["w"], c["scale"], c["antialiasing"]) for c in CASES] == WANT


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tables_equal_the_reference_bit_for_bit(case):
    n, s, aa = case["name"], case["scale"], case["antialiasing"]
    for ax, L, k in (("h", case["h"], 0), ("w", case["w"], 2)):
        w, src = R.weights_indices(L, R.out_length(L, s), s, aa)
        gw, gi = G[f"{n}_w{ax}"], G[f"{n}_i{ax}"]
        sym_s, sym_e = int(G[f"{n}_sym"][k]), int(G[f"{n}_sym"][k + 1])
        assert w.dtype == np.float32 and src.dtype == np.int32 and w.shape == gw.shape == src.shape == gi.shape
        assert np.array_equal(w.view(np.uint32), gw.view(np.uint32)), f"{n} {ax}: weights differ"
        pos = gi.astype(np.int64) - sym_s                      # the augmented index read as a position in the image
        want = np.where(pos < 0, -pos - 1, np.where(pos >= L, 2 * L - 1 - pos, pos))
        assert np.array_equal(src, want), f"{n} {ax}: indices differ"
        assert src.min() >= 0 and src.max() < L
        assert R.tables(L, R.out_length(L, s), s, aa)[2:] == (sym_s, sym_e)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pixels_within_the_derived_bound_of_the_reference(case):
    n, h, w, s, aa = case["name"], case["h"], case["w"], case["scale"], case["antialiasing"]
    img, ref = G[f"{n}_img"], G[f"{n}_out"]
    got = R.imresize_u8(img, s, aa)
    assert got.dtype == np.float32 and got.shape == (3, R.out_length(h, s), R.out_length(w, s))
    bound = R.error_bound(h, w, s, aa, max_abs=1.0)            # the input is in [0, 1]
    # the formula, restated from the tables
    wh, ww = G[f"{n}_wh"].astype(np.float64), G[f"{n}_ww"].astype(np.float64)
    sh, sw = np.abs(wh).sum(1).max(), np.abs(ww).sum(1).max()
    assert bound == pytest.approx((wh.shape[1] * sh + ww.shape[1] * sw * sh) * 2.0 ** -24, rel=1e-12)
    d = float(np.abs(got.transpose(1, 2, 0) - ref).max())
    print(f"RESIZE-DIFF {n}: max |resize.py - reference| {d:.3e} bound {bound:.3e}")
    assert d <= bound
    # layouts and the byte conversion
    assert np.array_equal(R.imresize(np.ascontiguousarray(R.u8_planes(img).transpose(1, 2, 0)), s, aa, layout="hwc"), got.transpose(1, 2, 0))
    assert np.array_equal(R.imresize_u8(img[:, :, ::-1], s, aa, bgr=True), got)
    v = np.clip(got, 0, 1) * np.float32(255.0)
    assert np.array_equal(R.to_u8(got), np.rint(v).astype(np.uint8).transpose(1, 2, 0))
    if s > 1:
        assert got.min() < 0 and got.max() > 1, "no clamp: the overshoot stays"


def test_a_flat_image_stays_flat_and_half_rounds_to_even():
    flat = np.full((3, 24, 36), np.float32(0.5), dtype=np.float32)
    out = R.imresize(flat, 0.25)
    assert np.abs(out - 0.5).max() <= 4e-7
    assert R.to_u8(np.array([[[0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0]]] * 3, dtype=np.float32)).tolist() == [[[0] * 3, [2] * 3, [2] * 3, [0] * 3, [255] * 3]]


@pytest.mark.parametrize("scale,aa", [(1 / 2, True), (1 / 3, True), (1 / 4, True), (0.75, True), (0.3, True), (2.0, True), (3.0, True), (1 / 2, False)])
def test_too_small_a_source_is_refused(scale, aa):
    """the smallest accepted length from the definition: sym_len_s = 1 - min(index), sym_len_e = max(index) - in_len, both <= in_len"""
    n0 = R.smallest_length(scale, aa)
    assert n0 >= 2
    for n in range(1, n0):
        with pytest.raises(ValueError, match="too small"):
            R.weights_indices(n, R.out_length(n, scale), scale, aa)
    # from there on: every index is inside the image.  At a scale that is no 1 / integer, ceil(n * scale) jumps and single
    # lengths above n0 can still need more mirror than they have (0.3: 6 is accepted, 7 is not); those are refused as well.
    whole = abs(round(max(scale, 1 / scale)) - max(scale, 1 / scale)) < 1e-9
    for n in range(n0, n0 + 40):
        try:
            _, src = R.weights_indices(n, R.out_length(n, scale), scale, aa)
        except ValueError:
            assert not whole and n > n0, f"length {n} is refused above the smallest accepted length {n0}"
            continue
        assert src.min() >= 0 and src.max() < n
    _, s, sym_s, sym_e = R.tables(n0, R.out_length(n0, scale), scale, aa)
    assert sym_s == -int(s.min()) and sym_e == int(s.max()) + 1 - n0 and max(sym_s, sym_e) <= n0


def _write(path, a):
    from super_resolution_amd.data import write_image
    write_image(a, str(path))


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_imagenet_paired_dataset(tmp_path, scale):
    from super_resolution_amd.data import FolderDataset, read_image
    rng = np.random.default_rng(31)
    sizes = [(50, 71), (33, 47)]
    for i, (h, w) in enumerate(sizes):
        _write(tmp_path / "gt" / f"im{i}.png", rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    ds = FolderDataset({"name": "Toy", "type": "ImageNetPairedDataset", "dataroot_gt": str(tmp_path / "gt"), "scale": scale, "phase": "test",
                        "io_backend": {"type": "disk"}})
    assert len(ds) == 2
    for i, d in enumerate(ds):
        h, w = sizes[i]
        H, W = h - h % scale, w - w % scale
        assert set(d) == {"lq", "gt", "gt_path", "lq_path"} and d["lq_path"] == d["gt_path"] == [str(tmp_path / "gt" / f"im{i}.png")]
        gt = read_image(d["gt_path"][0])[:, :H, :W]
        assert tuple(d["gt"].shape) == (1, 3, H, W) and tuple(d["lq"].shape) == (1, 3, H // scale, W // scale)
        assert d["lq"].dtype == d["gt"].dtype == torch.float32
        assert torch.equal(d["gt"][0], gt)
        assert np.array_equal(d["lq"][0].numpy(), R.imresize(np.ascontiguousarray(gt.numpy()), 1 / scale))
    base = {"name": "Toy", "type": "ImageNetPairedDataset", "dataroot_gt": str(tmp_path / "gt"), "scale": scale, "phase": "test"}
    for extra in ({"color": "y"}, {"mean": [0.5] * 3}, {"std": [0.5] * 3}, {"io_backend": {"type": "lmdb"}}, {"meta_info_file": "x.txt"},
                  {"phase": "train"}):
        with pytest.raises(NotImplementedError):
            FolderDataset(dict(base, **extra))
    with pytest.raises(ValueError, match="scale"):
        FolderDataset({k: v for k, v in base.items() if k != "scale"})
    with pytest.raises(RuntimeError, match="gt_size"):
        FolderDataset(dict(base, gt_size=48))[1]
    assert tuple(FolderDataset(dict(base, gt_size=32))[0]["gt"].shape) == (1, 3, 50 - 50 % scale, 71 - 71 % scale)


def test_parse_options_sets_lq_on_device(tmp_path):
    from super_resolution_amd.test import parse_options
    p = tmp_path / "o.yml"
    p.write_text("name: t\nscale: 4\ndatasets:\n  test_1:\n    name: A\n    type: ImageNetPairedDataset\n    dataroot_gt: gt\nval:\n  save_img: false\n")
    opt = parse_options(str(p), lq_on_device=True)
    assert opt["val"] == {"save_img": False, "u8_on_device": True, "lq_on_device": True}
    assert opt["datasets"]["test_1"]["scale"] == 4 and opt["datasets"]["test_1"]["phase"] == "test"
    assert "lq_on_device" not in parse_options(str(p))["val"]


PROTOTYPES = {
    "hat_imresize_rows": "const void* src, int32_t src_u8, int64_t src_pitch, int64_t src_bstride, int32_t bgr, float* mid, int32_t B, int32_t h, "
                         "int32_t w, int32_t oh, const float* w_h, const int32_t* src_h, int32_t P_h, int64_t n_table, void* stream",
    "hat_imresize_cols_to_planes": "const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w, const int32_t* src_w, "
                                   "int32_t P_w, int64_t n_table, float* dst, int32_t Hp, int32_t Wp, void* stream",
    "hat_imresize_cols_to_u8": "const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w, const int32_t* src_w, int32_t P_w, "
                               "int64_t n_table, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride, int32_t bgr, void* stream",
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_and_ctypes_prototypes_agree(name):
    from super_resolution_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hat_mi355x.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/hat_mi355x.h"
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(m.group(1)) == norm(PROTOTYPES[name])
    ctype = lambda a: C.c_void_p if "*" in a else {"int32_t": C.c_int32, "int64_t": C.c_int64}[a.split()[0]]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [ctype(a.strip()) for a in m.group(1).split(",")]


def test_lq_on_device_does_not_resize_on_the_host(tmp_path, monkeypatch):
    """Under val.lq_on_device the GT-only dataset must not make `lq`: the device makes it, and nothing would read the host's."""
    from super_resolution_amd.data import FolderDataset
    from super_resolution_amd.models import HATModel
    rng = np.random.default_rng(32)
    for i in range(2):
        _write(tmp_path / "gt" / f"im{i}.png", rng.integers(0, 256, (26, 34, 3), dtype=np.uint8))
    ds = FolderDataset({"name": "Toy", "type": "ImageNetPairedDataset", "dataroot_gt": str(tmp_path / "gt"), "scale": 4, "phase": "test"})
    calls = []
    real = R.imresize
    monkeypatch.setattr(R, "imresize", lambda *a, **k: calls.append(1) or real(*a, **k))
    seen = []

    def fake(self, val_data, metrics, save_img, on_device):
        seen.append(sorted(val_data))
        assert tuple(val_data["gt"].shape) == (1, 3, 24, 32)
        return {}, {}

    monkeypatch.setattr(HATModel, "_test_lq_on_device", fake)
    m = HATModel.__new__(HATModel)                      # no network: only the loop around the items is under test
    m.opt = {"name": "toy", "scale": 4, "val": {"lq_on_device": True, "metrics_on_device": True}}
    m.nondist_validation(ds, save_img=False)
    assert seen == [["gt", "gt_path", "lq_path"]] * 2 and calls == []
    assert ds.make_lq is True and "lq" in ds[0] and calls == [1]          # the float route still gets its LQ image
