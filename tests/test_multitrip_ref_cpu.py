"""The banded fp64 convolution and the chunked re-run that test_gpu_multitrip.py judges the kernels by, pinned on the CPU to
F.conv2d and to a direct loop: bands that do not divide the height, halos at the frame border, per-sample weights."""
import pytest
import torch
import torch.nn.functional as F

from helpers import conv_ref_banded, rnd, run_chunked


@pytest.mark.parametrize("k,band", [(3, 4), (3, 64), (13, 5), (5, 7)])
def test_conv_ref_banded_matches_conv2d(k, band):
    B, H, W, cin, cout = 2, 19, 23, 5, 7
    x = rnd(f"crx{k}", (B, H, W, cin))
    w = rnd(f"crw{k}", (cout, cin, k, k), std=0.2)
    b = rnd(f"crb{k}", (cout,), std=0.1)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1)
    got = conv_ref_banded(x, w, b, band=band)
    assert got.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-12
    wb = rnd(f"crwb{k}", (B, cout, cin, k, k), std=0.2)
    refb = torch.cat([F.conv2d(x[i:i + 1].permute(0, 3, 1, 2).double(), wb[i].double(), padding=k // 2) for i in range(B)], 0)
    assert float((conv_ref_banded(x, wb, band=band) - refb.permute(0, 2, 3, 1)).abs().max()) <= 1e-12


def test_run_chunked_covers_every_pixel_once_and_never_crosses_a_sample():
    B, N = 2, 37
    src = torch.arange(B * N * 3, dtype=torch.float32).reshape(B, N, 3)
    dst = torch.zeros_like(src)
    seen = []

    def launch(v, b):
        assert v["src"].shape[0] == 1 and v["src"].is_contiguous() and v["src"].shape[1] <= 16
        seen.append((b, v["src"].shape[1]))
        v["dst"] += v["src"]

    run_chunked(launch, dict(src=src, dst=dst), B, N, 16)
    assert torch.equal(dst, src) and seen == [(0, 16), (0, 16), (0, 5), (1, 16), (1, 16), (1, 5)]
