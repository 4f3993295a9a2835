"""The ESC-LTE benchmark loop without a device: the host restatement of Pillow's 8-bit bicubic resize against Pillow
(live where PIL imports, and always against tests/golden/pil_bicubic.npz), the byte <-> float round trip that lets the device start
from bytes, the wrappers' size / crop / cell arithmetic, metrics.arb_psnr against a restatement of the reference's formula, config
parsing and every refusal."""
import math

import numpy as np
import pytest
import torch

import arb_eval_cases as cases
from super_resolution_amd import arb_test, metrics, resize

NAMES = list(cases.RESIZE_CASES)


@pytest.fixture(scope="module")
def golden():
    return cases.golden()


@pytest.mark.parametrize("name", NAMES)
def test_host_resize_equals_the_golden_pillow(golden, name):
    (h, w), (oh, ow), _ = cases.RESIZE_CASES[name]
    src = cases.source(name)
    assert src.shape == (h, w, 3) and np.array_equal(golden[name + ".in"], src), "the golden file was made from another input"
    got = resize.pil_bicubic_u8(src, (oh, ow))
    assert got.dtype == np.uint8 and got.shape == (oh, ow, 3)
    assert np.array_equal(got, golden[name + ".out"])


@pytest.mark.parametrize("name", NAMES)
def test_host_resize_equals_live_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    _, (oh, ow), _ = cases.RESIZE_CASES[name]
    src = cases.source(name)
    want = np.asarray(Image.fromarray(src, "RGB").resize((ow, oh), Image.BICUBIC))
    assert np.array_equal(resize.pil_bicubic_u8(src, (oh, ow)), want)


def test_pil_tables_shape_and_sum():
    """K = 2 ceil(2 max(in / out, 1)) + 1: 121 at x30, 5 when enlarging; the fixed-point weights of a position sum to 2^22 within
    one unit per tap; the taps stay inside the source."""
    for n_in, n_out, K in ((600, 20, 121), (95, 3, 2 * math.ceil(2 * 95 / 3) + 1), (37, 48, 5), (9, 1, 37)):
        coef, bounds = resize.pil_tables(n_in, n_out)
        assert coef.shape == (n_out, K) and coef.dtype == np.int32 and bounds.shape == (n_out, 2) and bounds.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= K).all() and (bounds.sum(1) <= n_in).all()
        for i in range(n_out):
            assert abs(int(coef[i, :bounds[i, 1]].sum()) - (1 << 22)) <= bounds[i, 1]
            assert not coef[i, bounds[i, 1]:].any()
    with pytest.raises(ValueError):
        resize.pil_tables(0, 4)
    with pytest.raises(ValueError):
        resize.pil_bicubic_u8(np.zeros((4, 4, 3), np.float32), (2, 2))


def test_byte_float_round_trip_is_the_identity():
    """ToTensor's byte / 255 in fp32, then ToPILImage's x255 and truncation (what surrounds the reference's resize_fn), gives every
    byte back: the device may start from the bytes."""
    b = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(b.to(torch.float32).div(255).mul(255).byte(), b)


def test_wrapper_arithmetic():
    H, W = 101, 77
    for scale, lr, hr in ((2, (50, 38), (100, 76)), (3, (33, 25), (99, 75)), (6, (16, 12), (96, 72)), (3.5, (28, 22), (98, 77)),
                          (30, (3, 2), (90, 60))):
        got_lr, got_hr = arb_test.downsampled_sizes(H, W, scale)
        assert got_lr == tuple(math.floor(n / scale + 1e-9) for n in (H, W)) == lr
        assert got_hr == tuple(round(n * scale) for n in lr) == hr
    assert arb_test.downsampled_sizes(90, 60, 30) == ((3, 2), (90, 60))           # the 1e-9: 90 / 30 must not floor to 2
    assert arb_test.paired_sizes(25, 19, 101, 77) == (4, (100, 76))
    assert arb_test.paired_sizes(25, 19, 100, 76) == (4, (100, 76))
    with pytest.raises(ValueError):
        arb_test.paired_sizes(25, 20, 101, 77)    # s = 4 needs 80 columns
    with pytest.raises(ValueError):
        arb_test.paired_sizes(25, 19, 20, 77)     # s = 0
    with pytest.raises(ValueError):
        arb_test.downsampled_sizes(10, 10, 30)
    # the cell: the config's S against scale_max, never the image's own ratio
    assert arb_test.cell_factor(2, 4) == 1 and arb_test.cell_factor(4, 4) == 1 and arb_test.cell_factor(6, 4) == 1.5
    assert arb_test.cell_factor(4, 2) == 2 and arb_test.cell_factor(None, 4) == 1
    for S, smax in ((2, 4), (4, 4), (12, 4), (None, 4)):
        f = 1 if S is None else max(S / smax, 1)
        want = tuple(float((torch.ones(1) * (2 / n)) * f) for n in (100, 76))    # wrappers.py:70-72 then test.py:92, in fp32
        assert arb_test.eval_cells(100, 76, S, smax) == want


def test_eval_types():
    assert arb_test.parse_eval_type(None) == (None, 0, None)
    assert arb_test.parse_eval_type("benchmark-4") == ("benchmark", 4, 4)
    assert arb_test.parse_eval_type("div2k-12") == ("div2k", 18, 12)
    for bad in ("ssim-4", "bench-2", 4, "div2k", "benchmark-x"):
        with pytest.raises(NotImplementedError):
            arb_test.parse_eval_type(bad)


def reference_psnr(pred, gt_u8, dataset, scale):
    """The reference's score in fp32 torch: the prediction cut to the ground truth's size and clamped, the difference to
    byte / 255; 'benchmark' weights the channels of the difference by (65.738, 129.057, 25.064) / 256, adds them and shaves `scale`
    pixels; 'div2k' keeps the channels and shaves scale + 6; the mean of the squares, -10 log10."""
    h, w = gt_u8.shape[:2]
    sr = torch.from_numpy(pred)[None, :, :h, :w].clamp(0, 1)
    hr = torch.from_numpy(gt_u8).permute(2, 0, 1)[None].to(torch.float32) / 255
    diff = sr - hr
    if dataset == "benchmark":
        diff = (diff * (torch.tensor([65.738, 129.057, 25.064]).view(1, 3, 1, 1) / 256)).sum(dim=1)
        cut = scale
    elif dataset == "div2k":
        cut = scale + 6
    else:
        cut = 0
    if cut:
        diff = diff[..., cut:-cut, cut:-cut]
    return float(-10 * torch.log10(diff.pow(2).mean()))


psnr_pair = cases.psnr_pair


@pytest.mark.parametrize("mode,scale", [("benchmark", 4), ("div2k", 2), (None, 0)])
def test_arb_psnr_against_the_reference_formula(mode, scale):
    pred, gt = psnr_pair()
    shave = {"benchmark": scale, "div2k": scale + 6, None: 0}[mode]
    got, want = metrics.arb_psnr(pred, gt, mode, shave), reference_psnr(pred, gt, mode, scale)
    print(f"arb_psnr {mode}-{scale}: {got:.6f} dB against {want:.6f} dB")
    assert abs(got - want) <= 1e-3
    total, terms = metrics.arb_psnr_sums(pred, gt, mode, shave)
    assert terms == (40 - 2 * shave) * (56 - 2 * shave) * (1 if mode == "benchmark" else 3)
    # a larger prediction is cut to the ground truth's size
    big = np.pad(pred, ((0, 0), (0, 3), (0, 5)), constant_values=0.5)
    assert metrics.arb_psnr_sums(big, gt, mode, shave) == (total, terms)


def test_arb_psnr_refusals():
    pred, gt = psnr_pair(20, 24, 20, 24)
    assert metrics.arb_psnr_sums(pred, gt, "benchmark", 9)[1] == 2 * 6
    for shave in (10, 12, -1):
        with pytest.raises(ValueError):
            metrics.arb_psnr(pred, gt, "benchmark", shave)
    with pytest.raises(ValueError):
        metrics.arb_psnr(pred[:, :19], gt, None, 0)
    with pytest.raises(NotImplementedError):
        metrics.arb_psnr(pred, gt, "ssim", 0)
    assert metrics.arb_psnr(gt.transpose(2, 0, 1).astype(np.float32) / np.float32(255), gt, None, 0) == float("inf")


def test_library_refuses_a_shave_that_leaves_nothing():
    """hat_arb_psnr_workspace_bytes is a pure host query with hat_arb_psnr's size checks: HAT_EINVAL for 2 shave >= a side."""
    import ctypes as C
    from super_resolution_amd import _lib, build
    build.build(verbose=False)
    lib, n = _lib.load(), C.c_int64(0)
    assert lib.hat_arb_psnr_workspace_bytes(20, 24, 9, C.byref(n)) == 0 and n.value == 8
    assert lib.hat_arb_psnr_workspace_bytes(1020, 1356, 8, C.byref(n)) == 0 and n.value == 8 * 1024
    for h, w, shave in ((20, 24, 10), (24, 20, 10), (20, 24, -1), (0, 24, 0)):
        assert lib.hat_arb_psnr_workspace_bytes(h, w, shave, C.byref(n)) == -1
    assert lib.hat_arb_psnr(None, 20, 24, None, 72, 20, 24, 1, 10, None, None, None) == -1
    assert lib.hat_arb_psnr(None, 20, 24, None, 72, 20, 24, 1, 2, None, None, None) == -1      # null pointers
    assert lib.hat_pil_resize_u8(None, 0, 4, 4, None, None, 0, 2, 2, None, None, 5, None, None, 5, None) == -1


CONFIGS = {
    "paired": """
test_dataset:
  dataset:
    name: paired-image-folders
    args:
      root_path_1: {lr}
      root_path_2: {gt}
  wrapper:
    name: sr-implicit-paired
    args: {{}}
  batch_size: 1
eval_type: benchmark-4
eval_bsize: 300000

data_norm:
  inp: {{sub: [0.5], div: [0.5]}}
  gt: {{sub: [0.5], div: [0.5]}}
""",
    "downsampled": """
test_dataset:
  dataset:
    name: image-folder
    args:
      root_path: {gt}
  wrapper:
    name: sr-implicit-downsampled
    args:
      scale_min: 12
  batch_size: 1
eval_type: div2k-12
eval_bsize: 30000


data_norm:
  inp: {{sub: [0.5], div: [0.5]}}
  gt: {{sub: [0.5], div: [0.5]}}
""",
    "paired_fast": """
test_dataset:
  dataset:
    name: paired-image-folders
    args:
      root_path_1: {lr}
      root_path_2: {gt}
      first_k: 1
      repeat: 2
  wrapper:
    name: sr-implicit-paired-fast
    args: {{}}
  batch_size: 1
eval_type: div2k-2
eval_bsize: 300000

data_norm:
  inp: {{sub: [0.5], div: [0.5]}}
  gt: {{sub: [0.5], div: [0.5]}}
""",
}


def _config(tmp_path, name, **edit):
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load(CONFIGS[name].format(lr=tmp_path / "lr", gt=tmp_path / "gt"))
    for path, v in edit.items():
        node, keys = cfg, path.split("__")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return cfg


def test_config_parsing(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for d in ("lr", "gt"):
        (tmp_path / d).mkdir()
        for n in ("b.png", "a.png"):
            Image.fromarray(cases.noise(d + n, (8, 8, 3)), "RGB").save(tmp_path / d / n)
    p = arb_test.parse_config(_config(tmp_path, "paired"))
    assert (p["kind"], p["eval_type"], p["eval_bsize"], p["scale"], p["first_k"], p["repeat"]) == ("paired", "benchmark-4", 300000, None, None, 1)
    assert p["roots"] == (str(tmp_path / "lr"), str(tmp_path / "gt"))
    assert arb_test.list_items(p) == [(str(tmp_path / "lr" / n), str(tmp_path / "gt" / n)) for n in ("a.png", "b.png")]
    d = arb_test.parse_config(_config(tmp_path, "downsampled"))
    assert (d["kind"], d["eval_type"], d["scale"], d["roots"]) == ("downsampled", "div2k-12", 12, (str(tmp_path / "gt"),))
    assert arb_test.list_items(d) == [(str(tmp_path / "gt" / n),) for n in ("a.png", "b.png")]
    f = arb_test.parse_config(_config(tmp_path, "paired_fast"))
    assert (f["kind"], f["first_k"], f["repeat"]) == ("paired", 1, 2)
    assert arb_test.list_items(f) == [(str(tmp_path / "lr" / "a.png"), str(tmp_path / "gt" / "a.png"))] * 2
    assert torch.equal(arb_test.read_u8(str(tmp_path / "gt" / "a.png")), torch.from_numpy(cases.noise("gta.png", (8, 8, 3))))


def test_config_refusals(tmp_path):
    NI = NotImplementedError
    for name, edit, err in (
            ("paired", dict(data_norm__inp__sub=[0.0]), NI), ("paired", dict(data_norm__gt__div=[1.0]), NI), ("paired", dict(data_norm=None), NI),
            ("paired", dict(test_dataset__wrapper__args=dict(inp_size=48)), NI), ("paired", dict(test_dataset__wrapper__args=dict(augment=True)), NI),
            ("downsampled", dict(test_dataset__wrapper__args=dict(scale_min=2, sample_q=2304)), NI),
            ("downsampled", dict(test_dataset__wrapper__args=dict(scale_min=1, scale_max=4)), NI),
            ("downsampled", dict(test_dataset__wrapper__name="sr-implicit-uniform-varied"), NI),
            ("downsampled", dict(test_dataset__wrapper__name="sr-implicit-paired"), ValueError),
            ("paired", dict(test_dataset__wrapper__name="sr-implicit-downsampled-fast"), ValueError),
            ("paired", dict(eval_type="ssim-4"), NI), ("paired", dict(test_dataset__dataset__args__cache="bin"), NI),
            ("paired", dict(test_dataset__dataset__args__split_file="split.json"), NI)):
        with pytest.raises(err):
            arb_test.parse_config(_config(tmp_path, name, **edit))
    assert arb_test.parse_config(_config(tmp_path, "paired", eval_type=None))["eval_type"] is None
    assert arb_test.parse_config(_config(tmp_path, "downsampled", test_dataset__wrapper__args=dict(scale_min=3, scale_max=3)))["scale"] == 3


def test_other_refusals(tmp_path, capsys):
    with pytest.raises(ValueError, match="17"):
        arb_test.check_lr_size(16, 40)
    arb_test.check_lr_size(17, 17)
    with pytest.raises(SystemExit):
        arb_test.main(["--config", "c.yaml", "--model", "m.pth", "--window", "8"])
    assert "window" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        arb_test.main(["--help"])
    out = capsys.readouterr().out
    assert "eval_bsize" in out and "--fast" in out and "do not change the arithmetic" in " ".join(out.split())
    # the model's calls refuse before any device work
    import super_resolution_amd.archs  # noqa: F401
    from super_resolution_amd.archs.esc_lte_arch import ESCLTE
    net = ESCLTE(n_blocks=1, conv_blocks=1).eval()
    with pytest.raises(RuntimeError, match="uint8"):
        net.score_u8(torch.zeros(20, 24, 3), torch.zeros(40, 48, 3, dtype=torch.uint8), eval_type="benchmark-2")
    with pytest.raises(RuntimeError, match="GPU"):
        net.score_gt_u8(torch.zeros(40, 48, 3, dtype=torch.uint8), 2, eval_type="benchmark-2")
