"""The 4:2:0 C entry points are adapters over the surface entry points: for a (1,1) surface both write the same bytes.  Each test
runs one operation through ops.yuv420_* (hat_yuv420[p16]_to_planes, hat_planes_to_yuv420[p16], hat_conv3x3_to_yuv420[p16]) and
through ops.yuv_* with sub=(1, 1) (hat_yuv_to_planes, hat_planes_to_yuv, hat_conv3x3_to_yuv) on the same views and inputs and asks
for equality; the definition itself is pinned elsewhere (test_gpu_yuv.py, test_gpu_yuv_deep.py, test_gpu_chroma.py)."""
import numpy as np
import pytest
import torch

from super_resolution_amd import yuv

pytestmark = pytest.mark.gpu
FMTS = ("nv12", "i420")                      # chroma step 2 and 1
DEPTHS = [(8, False), (10, True)]
DEPTH_IDS = ["8", "10msb"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _frame(seed, B, h, w, depth, dev):
    """Random stored samples of a (B, 3h/2, w) frame; deep words carry low bits under the MSB-aligned code."""
    a = np.random.default_rng(seed).integers(0, 256 if depth == 8 else 65536, (B,) + yuv.frame_shape(h, w))
    if depth == 8:
        return torch.from_numpy(a.astype(np.uint8)).to(dev)
    return torch.from_numpy(a.astype(np.uint16).view(np.int16)).to(dev).view(torch.uint16)


def _filled(B, h, w, depth, dev, fill):
    t = torch.full((B,) + yuv.frame_shape(h, w), fill, dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
    return t if depth == 8 else t.view(torch.uint16)


def _same(a, b):
    return torch.equal(a, b) if a.dtype == torch.uint8 else torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_to_planes_legacy_entry_is_the_surface_entry(fmt, dm):
    """A 6 x 10 frame into 8 x 16 planes: reflection on both axes, the pad smaller than the size."""
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    B, h, w, Hp, Wp = 2, 6, 10, 8, 16
    views = ops.yuv420_views(_frame(h * w + depth, B, h, w, depth, dev), fmt)
    m = yuv.csc("bt709", False, depth)[0]
    a, b = torch.full((B, 3, Hp, Wp), -7.0, device=dev), torch.full((B, 3, Hp, Wp), -9.0, device=dev)
    ops.yuv420_to_planes(*views, a, m, depth=depth, msb=msb)
    ops.yuv_to_planes(*views, b, m, sub=(1, 1), depth=depth, msb=msb)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", [(8, 16, 6, 10), (2, 1040, 2, 1030)], ids=["8x16_to_6x10", "2x1040_to_2x1030"])
def test_from_planes_legacy_entry_is_the_surface_entry(shape, fmt, dm):
    """A crop on both axes; a second block along x (a block takes 1024 columns) with a crop inside it."""
    dev = _dev()
    from super_resolution_amd import ops
    depth, msb = dm
    Hs, Ws, h, w = shape
    B = 2
    planes = torch.rand(B, 3, Hs, Ws, generator=torch.Generator().manual_seed(Ws + depth)).to(dev) * 1.2 - 0.1   # clamps on both ends
    m = yuv.csc("bt709", True, depth)[1]
    a, b = _filled(B, h, w, depth, dev, 77), _filled(B, h, w, depth, dev, 55)
    ops.planes_to_yuv420(planes, *ops.yuv420_views(a, fmt), m, depth=depth, msb=msb)
    ops.planes_to_yuv(planes, *ops.yuv420_views(b, fmt), m, sub=(1, 1), depth=depth, msb=msb)
    torch.cuda.synchronize()
    assert _same(a, b)


@pytest.mark.parametrize("dm", DEPTHS, ids=DEPTH_IDS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", [(24, 16, 24, 16), (24, 48, 22, 42)], ids=["24x16", "24x48_to_22x42"])
def test_conv_last_epilogue_legacy_entry_is_the_surface_entry(shape, fmt, dm):
    """One unit wide at full size; a crop inside a 16-column group and at an even-height band edge.  Input and packed weights as
    test_conv3x3_to_yuv_equals_planes_then_convert builds them."""
    dev = _dev()
    from super_resolution_amd import ops
    from super_resolution_amd.engine import RGB_MEAN
    depth, msb = dm
    H, W, ho, wo = shape
    B = 2
    g = torch.Generator().manual_seed(W)
    x = (torch.randn(B, H, W, 64, generator=g)).to(torch.bfloat16).to(dev)
    wl = torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0)
    bl = torch.randn(3, generator=g) * 0.1
    wpk, b8 = ops.pack_cab_squeeze(wl, bl, dev)
    kw = dict(B=B, H=H, W=W, C_=64, ldx=64, out_scale=0.5, mean=RGB_MEAN, dtype=ops.HAT_BF16, from_rgb=yuv.csc("bt709", True, depth)[1],
              depth=depth, msb=msb)
    a, b = _filled(B, ho, wo, depth, dev, 77), _filled(B, ho, wo, depth, dev, 55)
    ops.conv3x3_to_yuv420(x, wpk, b8, *ops.yuv420_views(a, fmt), **kw)
    ops.conv3x3_to_yuv(x, wpk, b8, *ops.yuv420_views(b, fmt), sub=(1, 1), **kw)
    torch.cuda.synchronize()
    assert _same(a, b)
