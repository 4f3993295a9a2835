"""NIQE block sums on the GPU (csrc/hat_niqe.hip, ops.niqe_stats, metrics_device.calculate_niqe_u8, `val.metrics_on_device` on
a dataset without ground truth) against the host definition super_resolution_amd/niqe.py and the reference's recorded scores
(tests/golden/niqe.npz).  Bars, none of them taken from what a kernel returns (niqe_cases.py, test_niqe_cpu.py):
  Y plane      equals niqe.y_plane bit for bit
  half size    equals niqe.half_plane (resize.imresize) bit for bit: the bar tests/test_gpu_resize.py uses (torch.equal)
  counts       all ten per block equal the host's exactly.  A sign is fixed by fp32 roundings of fp64 sums; a flip would
               need an fp64 sum within 1e-16 of a rounding boundary.  A mismatch prints the block: it is not to be loosened.
  sums         the 15 sums per block and scale against fp64 sums of the host definition's fp32 maps: relative 1.33e-6 =
               10 x the 1.33e-7 that float32 and fp64 summation of the same values differ by over the golden images
  score        against the host definition and against the reference's score: 1.21e-5 = 10 x the 1.21e-6 that the host
               definition moves by between float32 and fp64 block sums (scores 9.8 to 18.4).  On the image `smooth` the
               reference's float64 route lies 8.5e-3 away, 700 bars: the device must sit on the float32 side.
Every test prints the differences it saw before it asserts (`pytest -s`)."""
import numpy as np
import pytest
import torch

from niqe_cases import COUNT_COLUMNS, SCORE_BAR, SUM_BAR, SUM_COLUMNS, checkerboard_frame, golden, noise_frame
from super_resolution_amd import metrics as M, niqe, synth

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def frames(g):
    """name -> (uint8 frame, crop_border): the golden images and the extra sizes; 96x96 is one block, 203x301 crops twice."""
    out = {c["name"]: (g[c["name"] + "_img"], c["crop_border"]) for c in g["cases"]}
    out.update({"one_block": (noise_frame(96, 96, 11), 0), "noise192": (noise_frame(192, 288, 12), 0),
                "odd_crop": (noise_frame(203, 301, 13), 4), "checker": (checkerboard_frame(), 0)})
    return out


@pytest.fixture(scope="module")
def host(frames):
    """name -> the host definition's plane, half plane and fp64-sum stats; computed once and left unchanged."""
    out = {}
    for name, (img, crop) in frames.items():
        plane = niqe.y_plane(img, crop)
        half = niqe.half_plane(plane)
        out[name] = {"plane": plane, "half": half,
                     "stats": (niqe.block_stats(niqe.mscn(plane), 96, np.float64), niqe.block_stats(niqe.mscn(half), 48, np.float64))}
    return out


def _check_stats(tag, got, want):
    for scale, (a, b) in enumerate(zip(got, want), 1):
        assert a.shape == b.shape, (tag, a.shape, b.shape)
        bad = np.argwhere(a[..., COUNT_COLUMNS] != b[..., COUNT_COLUMNS])
        for i, j, k in bad[:8]:
            print(f"NIQE-COUNT {tag} scale {scale} block ({i},{j}) column {COUNT_COLUMNS[k]}: device {a[i, j, COUNT_COLUMNS[k]]!r} host {b[i, j, COUNT_COLUMNS[k]]!r}")
        with np.errstate(all="ignore"):
            rel = np.where(b[..., SUM_COLUMNS] == 0, np.abs(a[..., SUM_COLUMNS]), np.abs(a[..., SUM_COLUMNS] - b[..., SUM_COLUMNS]) / np.abs(b[..., SUM_COLUMNS]))
        print(f"NIQE-SUMS {tag} scale {scale}: {a.shape[0]}x{a.shape[1]} blocks, count mismatches {len(bad)}, largest relative sum difference {rel.max():.3e} (bar {SUM_BAR:.3e})")
        assert len(bad) == 0, tag
        assert rel.max() <= SUM_BAR, tag


def test_planes_and_block_sums(frames, host):
    from super_resolution_amd import ops
    dev = _dev()
    for name, (img, crop) in frames.items():
        s96, s48 = ops.niqe_stats(torch.from_numpy(img).to(dev), crop_border=crop)
        buf = ops._niqe_buffers_for(dev, 1, img.shape[0], img.shape[1], crop)
        plane, half = buf["plane"][0].cpu().numpy(), buf["half"][0].cpu().numpy()
        assert np.array_equal(plane, host[name]["plane"]), f"{name}: Y plane"
        assert np.array_equal(buf["unit"][0].cpu().numpy(), host[name]["plane"] / np.float32(255.0)), f"{name}: / 255 copy"
        assert np.array_equal(half, host[name]["half"]), f"{name}: half-size plane"
        _check_stats(name, (s96[0].cpu().numpy(), s48[0].cpu().numpy()), host[name]["stats"])


def test_batch_pitch_and_bgr(frames, host):
    """B = 2 with pitched rows and a sample stride, and the B, G, R byte order: the same sums as one frame at a time."""
    from super_resolution_amd import ops
    dev = _dev()
    a, b = frames["noise192"][0], frames["checker"][0]
    big = torch.zeros(2, 200, 300, 3, dtype=torch.uint8, device=dev)
    view = big[:, :192, :288]
    view[0], view[1] = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    s96, s48 = ops.niqe_stats(view, crop_border=0)
    got = (s96.cpu().numpy(), s48.cpu().numpy())
    for i, name in enumerate(("noise192", "checker")):
        _check_stats(f"batch[{i}] {name}", (got[0][i], got[1][i]), host[name]["stats"])
    r96, r48 = ops.niqe_stats(torch.from_numpy(np.ascontiguousarray(a[:, :, ::-1])).to(dev), crop_border=0, bgr=True)
    assert np.array_equal(r96[0].cpu().numpy(), got[0][0]) and np.array_equal(r48[0].cpu().numpy(), got[1][0])
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.niqe_stats(torch.zeros(95, 200, 3, dtype=torch.uint8, device=dev), crop_border=0)


def test_scores_against_the_reference_and_the_host(g, frames):
    from super_resolution_amd.metrics_device import calculate_metrics_u8, calculate_niqe_u8
    dev = _dev()
    for c in g["cases"]:
        name, crop = c["name"], c["crop_border"]
        opt = {"type": "calculate_niqe", "crop_border": crop, "pris_params": g["pris"]}
        got = calculate_niqe_u8(torch.from_numpy(g[name + "_img"]).to(dev), opt)
        want_ref, want_host = float(g[name + "_score"]), M.calculate_metric({"img": g[name + "_img"]}, opt)
        print(f"NIQE-SCORE {name}: device {got!r} host {want_host!r} reference {want_ref!r} |d host| {abs(got - want_host):.3e} |d reference| "
              f"{abs(got - want_ref):.3e} (bar {SCORE_BAR:.3e}; float64 route {float(g[name + '_score64'])!r})")
        if np.isnan(want_ref):
            assert np.isnan(got) and np.isnan(want_host), name
        else:
            assert abs(got - want_host) <= SCORE_BAR and abs(got - want_ref) <= SCORE_BAR, name
    img = frames["checker"][0]
    opt = {"type": "calculate_niqe", "crop_border": 0, "pris_params": g["pris"]}
    both = calculate_metrics_u8(torch.from_numpy(img).to(dev), None, {"niqe": opt}, niqe=True)
    assert calculate_metrics_u8(torch.from_numpy(img).to(dev), None, {"niqe": opt}) == {}   # without niqe=True: left out, as before
    want = M.calculate_metric({"img": img}, opt)
    print(f"NIQE-SCORE checker: device {both['niqe']!r} host {want!r} |d| {abs(both['niqe'] - want):.3e}")
    assert np.isfinite(want) and abs(both["niqe"] - want) <= SCORE_BAR
    with pytest.raises(RuntimeError, match="need the second frame"):
        calculate_metrics_u8(torch.from_numpy(img).to(dev), None, {"psnr": {"type": "calculate_psnr", "crop_border": 0}})


@pytest.mark.parametrize("tile", [None, {"tile_size": 32, "tile_pad": 16}], ids=["whole", "tiled"])
def test_harness_niqe_without_ground_truth(g, tmp_path, tile):
    """A SingleImageDataset (no gt) with a NIQE-only val.metrics: metrics_on_device scores the result where it lies and gives
    the host route's value on the downloaded uint8 result."""
    dev = _dev()
    from oracle import hat_oracle as O
    from super_resolution_amd import data as D
    from super_resolution_amd.models import HATModel
    netopt = dict(type="HAT", upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=4, squeeze_factor=4, conv_scale=0.01,
                  overlap_ratio=0.5, img_range=1.0, depths=[2], embed_dim=24, num_heads=[2], mlp_ratio=2, upsampler="pixelshuffle",
                  resi_connection="1conv", compute_dtype="bf16")
    for i, (h, w) in enumerate([(101, 150), (53, 101)]):    # results 202x300 and 106x202: 2x3 blocks and 1x2 blocks after crop 4
        D.write_image(noise_frame(h, w, 80 + i), str(tmp_path / "lq" / f"im{i}.png"))
    cfg = O.make_cfg(**{k: v for k, v in netopt.items() if k not in ("type", "compute_dtype")})
    torch.save({"params": synth.synth_state_dict(O.blank_state_dict(cfg), 21)}, tmp_path / "net.pth")
    metrics = {"niqe": {"type": "calculate_niqe", "crop_border": 4, "pris_params": g["pris"]}}

    def run(vis, save, **val):
        opt = {"name": "toy", "scale": 2, "network_g": dict(netopt), "path": {"visualization": str(tmp_path / vis), "pretrain_network_g": str(tmp_path / "net.pth")},
               "val": dict({"suffix": None, "metrics": metrics}, **val)}
        if tile:
            opt["tile"] = tile
        ds = D.FolderDataset({"name": "Toy", "type": "SingleImageDataset", "dataroot_lq": str(tmp_path / "lq"), "phase": "test"})
        return HATModel(opt, device=str(dev)).nondist_validation(ds, save_img=save)
    want_mean, want_rows = run("vis_u8", True, u8_on_device=True)            # the host route on the downloaded uint8 result
    got_mean, got_rows = run("vis_dev", False, metrics_on_device=True)
    assert not (tmp_path / "vis_dev").exists()
    for i in range(2):
        d = abs(got_rows[i]["niqe"] - want_rows[i]["niqe"])
        print(f"NIQE-HARNESS {'tiled' if tile else 'whole'} im{i}: host {want_rows[i]['niqe']!r} device {got_rows[i]['niqe']!r} |d| {d:.3e}")
        assert np.isfinite(want_rows[i]["niqe"]) and d <= SCORE_BAR
    assert abs(got_mean["niqe"] - want_mean["niqe"]) <= SCORE_BAR
