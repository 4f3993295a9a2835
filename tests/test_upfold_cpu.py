"""The host fold of Conv2d(64, 256, 3) -> PixelShuffle(2) -> Conv2d(64, 3, 3) into one 5x5 conv at the shuffle's input size
(packing.upfold_pieces / upfold_variant / upfold_apply), in fp64 against the composition in torch: every output pixel,
borders and corners included; and the interior formula alone must be wrong on the border ring (the zero padding of the SHUFFLED
map removes whole shifts there, which zero padding of x does not reproduce)."""
import pytest
import torch
import torch.nn.functional as F

from super_resolution_amd import packing

SIZES = [(1, 1), (1, 5), (2, 2), (3, 7), (6, 6)]   # (H, W) of the shuffle's input


def _weights(seed, c=8, k=5, m=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(4 * k, c, 3, 3), r(4 * k), r(m, k, 3, 3), r(m)


def _composition(x, wu, bu, wl, bl):
    return F.conv2d(F.pixel_shuffle(F.conv2d(x, wu, bu, padding=1), 2), wl, bl, padding=1)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fold_equals_the_composition_at_every_pixel(size):
    H, W = size
    wu, bu, wl, bl = _weights(11 + H * 16 + W)
    x = torch.randn(2, wu.shape[1], H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ref = _composition(x, wu, bu, wl, bl)
    got = packing.upfold_apply(x, wu, bu, wl, bl)
    assert got.shape == ref.shape == (2, 3, 2 * H, 2 * W)
    assert _rel(got, ref) <= 1e-10
    # the per-shift formula itself, not through the merged variants: shift the 3x3 result of every piece, absent outside the image
    G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
    acc = b0.repeat_interleave(4)[None, :, None, None].expand(2, 12, H, W).clone()
    for iy in range(3):
        for ix in range(3):
            t = F.conv2d(x, G[iy, ix].reshape(12, -1, 3, 3), Bd[iy, ix].reshape(-1), padding=1)
            t = F.pad(t, (1, 1, 1, 1))[:, :, iy:iy + H, ix:ix + W]       # t[p + delta], zero (absent) outside
            acc += t
    assert _rel(F.pixel_shuffle(acc, 2), ref) <= 1e-10


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_interior_formula_alone_is_wrong_on_the_border_ring(size):
    H, W = size
    wu, bu, wl, bl = _weights(3 + H * 16 + W)
    x = torch.randn(1, wu.shape[1], H, W, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    ref = _composition(x, wu, bu, wl, bl)
    G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
    Fi, bias = packing.upfold_variant(G, Bd, b0, 0, 0)
    y = F.pixel_shuffle(F.conv2d(x, Fi.reshape(12, -1, 5, 5), bias.reshape(-1), padding=2), 2)
    err = (y - ref).abs().amax(dim=(0, 1)) / ref.abs().max()
    ring = torch.ones(2 * H, 2 * W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False          # output pixels that touch the image border: the only ones a shift is absent for
    assert float(err[~ring].max()) <= 1e-10 if (~ring).any() else True
    assert float(err[ring].min()) > 1e-6, "every pixel of the ring loses a shift the interior weights still contain"


def test_packed_variants_hold_the_fold_in_mfma_order():
    g = torch.Generator().manual_seed(9)
    wu, bu = torch.randn(256, 64, 3, 3, generator=g) * 0.05, torch.randn(256, generator=g) * 0.1
    wl, bl = torch.randn(3, 64, 3, 3, generator=g) * 0.05, torch.randn(3, generator=g) * 0.1
    p = packing.pack_upfold(wu, bu, wl, bl, "cpu")
    assert p.w.shape == (12, 50, 64, 8) and p.w.dtype == torch.bfloat16 and p.bias.shape == (12, 16)
    G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
    for rs, cs in ((0, 0), (1, 2), (3, 1)):
        Fv, bias = packing.upfold_variant(G, Bd, b0, rs, cs)
        v = 3 * rs + cs
        for lane, t, ks, j in ((0, 0, 0, 0), (21, 12, 1, 3), (63, 24, 1, 7), (46, 7, 0, 5)):
            row, c = lane & 15, 32 * ks + 8 * (lane >> 4) + j
            ab, m = row >> 2, row & 3
            want = 0.0 if m == 3 else float(Fv[m, ab >> 1, ab & 1, c, t // 5, t % 5])
            assert float(p.w[v, 2 * t + ks, lane, j]) == float(torch.tensor(want, dtype=torch.float32).to(torch.bfloat16))
        assert torch.equal(p.bias[v].reshape(4, 4)[:, :3], bias.permute(1, 2, 0).reshape(4, 3).to(torch.float32))
        assert float(p.bias[v].reshape(4, 4)[:, 3].abs().max()) == 0.0
