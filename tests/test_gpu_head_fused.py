"""hat_head_fused (csrc/hat_head.hip): conv_first, the patch-embed LayerNorm and the first block's norm1 in one launch.

The kernel keeps hat_conv's k order and hat_layernorm's formula, summation tree and pixel partition, so everything it
writes — f0, t, n, the compact 16-channel copy, the GAP partials — must EQUAL what the three launches write (torch.equal, no
tolerance), at the kernel, through the engine and through a replayed plan."""
import os
from unittest import mock

import pytest
import torch

from helpers import META, W_SEED, X_SEED
from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

C = 144
TRIP = 1024 * 16   # pixels of one sample that one trip of the 1024 chains covers (hat_layernorm_blocks() * 16)
# exact tile; ragged right edge with several tiles a row; B > 1 with tiles that straddle rows; ragged bottom edge; then two
# shapes past one and two trips of the tile loop (the input is fetched two tiles ahead), ragged against the trip
SHAPES = [(1, 16, 16), (1, 17, 35), (2, 8, 50), (1, 33, 16), (1, 129, 130), (2, 181, 183)]
MEAN, RANGE = (0.4488, 0.4371, 0.4040), 1.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _params(dev, seed=7):
    from super_resolution_amd import ops
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, lo=-1.0, hi=1.0: torch.rand(*s, generator=g) * (hi - lo) + lo
    pw = ops.pack_conv_weight(r(C, 3, 3, 3, lo=-0.4, hi=0.4), r(C, lo=-0.2, hi=0.2), ops.HAT_BF16, dev)
    ln = [(r(C, lo=0.5, hi=1.5).to(dev), r(C, lo=-0.3, hi=0.3).to(dev)) for _ in range(2)]
    return pw, ln


def _three(pw, ln, x, gap_c):
    """The three launches of the engine's unfused head and first prologue."""
    from super_resolution_amd import ops
    B, _, H, W = x.shape
    dev, N = x.device, H * W
    f0, t = (torch.full((B, N, C), 7.0, device=dev) for _ in range(2))
    n = torch.full((B, N, C), 7.0, dtype=torch.bfloat16, device=dev)
    gap = torch.full((B, ops.layernorm_blocks(), 16), 7.0, device=dev)
    ops.conv(pw, x, f0, B=B, H=H, W=W, dtype=ops.HAT_BF16, ldx=0, ldo=C, x_mode=ops.X_NCHW_F32_MEAN, out_mode=ops.O_NHWC_F32,
             in_scale=RANGE, mean=MEAN)
    ops.layernorm(f0, t, *ln[0], B=B, npix=N, C_=C, ldy=C, out_f32=True, dtype=ops.HAT_BF16)
    ops.layernorm(t, n, *ln[1], B=B, npix=N, C_=C, ldy=C, out_f32=False, dtype=ops.HAT_BF16, gap=gap, gap_c=gap_c)
    torch.cuda.synchronize()
    return f0, t, n, gap


def _fused(pw, ln, x, gap_c):
    from super_resolution_amd import ops
    B, _, H, W = x.shape
    dev, N = x.device, H * W
    f0, t = (torch.full((B, N, C), 9.0, device=dev) for _ in range(2))
    n = torch.full((B, N, C), 9.0, dtype=torch.bfloat16, device=dev)
    n16 = torch.full((B, N, 16), 9.0, dtype=torch.bfloat16, device=dev)
    gap = torch.full((B, ops.layernorm_blocks(), 16), 9.0, device=dev)
    assert ops.head_fused_supported(pw, C, gap_c, ops.HAT_BF16)
    ops.head_fused(pw, x, f0, t, n, ln[0], ln[1], B=B, H=H, W=W, ldn=C, dtype=ops.HAT_BF16, in_scale=RANGE, mean=MEAN, n16=n16,
                   gap=gap, gap_c=gap_c)
    torch.cuda.synchronize()
    return f0, t, n, gap, n16


def _compare(x, gap_c=16):
    pw, ln = _params(x.device)
    f0, t, n, gap = _three(pw, ln, x, gap_c)
    g0, gt, gn, ggap, gn16 = _fused(pw, ln, x, gap_c)
    assert torch.isfinite(t).all() and float(t.abs().max()) > 0.5     # the case is not degenerate
    for name, a, b in (("f0", g0, f0), ("t", gt, t), ("n", gn, n), ("n16", gn16, n[..., :16].contiguous()), ("gap", ggap, gap)):
        diff = (a.float() - b.float()).abs().max().item()
        print(f"{tuple(x.shape)} gap_c={gap_c} {name}: max |fused - three launches| = {diff:.3e}")
        assert torch.equal(a, b), f"{name} differs from the three-launch result (max {diff:.3e}) at {tuple(x.shape)}"
    return gn, ggap


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_three_launches(shape):
    dev = _dev()
    B, H, W = shape
    _compare(synth.synth_input(X_SEED + 3, (B, 3, H, W)).to(dev))


@pytest.mark.parametrize("gap_c", [0, 4, 12])
def test_kernel_pools_the_channels_it_is_asked_for(gap_c):
    """gap_c < 16 (narrower ESC) and 0 (no pool: the partials buffer is not touched — both routes leave their fill)."""
    dev = _dev()
    from super_resolution_amd import ops
    x = synth.synth_input(X_SEED + 4, (1, 3, 17, 35)).to(dev)
    if gap_c:
        _compare(x, gap_c)
        return
    pw, ln = _params(dev)
    B, _, H, W = x.shape
    t, n = torch.zeros(B, H * W, C, device=dev), torch.zeros(B, H * W, C, dtype=torch.bfloat16, device=dev)
    ops.head_fused(pw, x, None, t, n, ln[0], ln[1], B=B, H=H, W=W, ldn=C, dtype=ops.HAT_BF16, in_scale=RANGE, mean=MEAN)   # no f0, n16, gap
    ref = _three(pw, ln, x, 16)
    assert torch.equal(t, ref[1]) and torch.equal(n, ref[2])


def test_border_ring_input():
    """Non-zero only on the outermost pixel ring: a halo read that wraps to the neighbouring row, or a tap outside the image
    that is not zeroed (the padding is zero AFTER the mean shift), changes the result."""
    dev = _dev()
    x = torch.zeros(1, 3, 17, 35)
    ring = synth.synth_input(X_SEED + 5, (1, 3, 17, 35))
    x[..., 0, :], x[..., -1, :], x[..., :, 0], x[..., :, -1] = ring[..., 0, :], ring[..., -1, :], ring[..., :, 0], ring[..., :, -1]
    _compare(x.to(dev))


@pytest.mark.parametrize("shape", [(1, 17, 35), (2, 8, 50)], ids=lambda s: "x".join(map(str, s)))
def test_gap_partials_pool_the_stored_rows(shape):
    """sum(partials) = sum over the pixels of the STORED bf16 n.  Every partial is a chain of at most trips + 16 fp32 additions
    (one per trip in a lane, then the 16 pixel slots in order; the partials themselves are added in fp64 here), so the
    error is at most (trips + 16) * 2^-24 * sum|n| per channel.  Pooling the unrounded values instead misses by about
    sqrt(N) * 2^-9 * |n|, two orders of magnitude more at these sizes."""
    dev = _dev()
    B, H, W = shape
    n, gap = _compare(synth.synth_input(X_SEED + 6, (B, 3, H, W)).to(dev))
    trips = -(-H * W // TRIP)
    want = n.double()[..., :16].sum(1)
    bound = (trips + 16) * 2.0 ** -24 * n.double()[..., :16].abs().sum(1)
    got = gap.double().sum(1)
    print(f"{shape}: max |sum(partials) - sum(n)| = {(got - want).abs().max().item():.3e}, smallest bound {bound.min().item():.3e}")
    assert ((got - want).abs() <= bound).all()


def _net(dev, env=None):
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(type="HAT", compute_dtype="bf16", **META["cfgs"]["hats_1g_x4"])).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    net = net.to(dev)
    with mock.patch.dict(os.environ, env or {}):   # (the engine reads its switches once, when it is built)
        net.engine()
    return net


def _launches(net, x):
    """The kernel names of one forward, in launch order (ops.profile brackets every launch)."""
    from super_resolution_amd import ops
    with ops.profile() as rec:
        net(x)
        torch.cuda.synchronize()
        return [r[0] for r in rec]


def test_engine_route_and_launch_count():
    """hats_1g_x4 (embed_dim 144, bf16): the default engine takes the fused head, HAT_NO_HEAD_FUSED=1 the three launches; the
    forwards are equal (which clears the 44 dB bar of test_fused_launches_agree_with_the_unfused_sequence with room), also
    for a batch and for a frame ragged against the 16-pixel tiles' rows."""
    dev = _dev()
    fused, plain = _net(dev), _net(dev, {"HAT_NO_HEAD_FUSED": "1"})
    assert fused.engine().head_fused and not plain.engine().head_fused
    for shape in ((1, 3, 32, 48), (2, 3, 16, 16)):
        x = synth.synth_input(X_SEED + 2, shape).to(dev)
        assert torch.equal(fused(x), plain(x)), shape
    x = synth.synth_input(X_SEED + 2, (1, 3, 32, 48)).to(dev)
    lf, lp = _launches(fused, x), _launches(plain, x)
    assert lf[0] == "head_fused_kernel" and lf[1] != "ln_kernel"
    assert lp[0].startswith("conv_kernel") and lp[1:3] == ["ln_kernel", "ln_kernel"]
    assert lp[3:] == lf[1:] and len(lp) - len(lf) == 2       # three launches became one; nothing else moved


def test_routes_that_keep_the_three_launches():
    """embed_dim 180 and the fp32 path are not fused."""
    dev = _dev()
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    for name, dtype in (("hat_1g_x2", "bf16"), ("hats_1g_x4", "f32")):
        net = build_network(dict(type="HAT", compute_dtype=dtype, **META["cfgs"][name])).eval().to(dev)
        assert not net.engine().head_fused, (name, dtype)


def test_plan_of_an_engine_with_the_fused_head(tmp_path):
    """The plan format's function table is fixed (its size is part of the file format), so the recorder takes the head as its
    three launches; the replay must still equal the eager forward, which runs hat_head_fused — and the engine is back on the
    fused route afterwards."""
    dev = _dev()
    from super_resolution_amd import plan
    net, shape = _net(dev), (1, 3, 16, 32)
    path = str(tmp_path / "net.hatplan")
    info = plan.export_plan(net, shape, path)
    assert "hat_head_fused" not in plan.FN_IDS and "hat_layernorm" in info["functions"]
    assert net.engine().head_fused
    x = synth.synth_input(X_SEED + 1, shape).to(dev)
    assert _launches(net, x)[0] == "head_fused_kernel"
    ref = net(x).clone()
    p = plan.Plan(path)
    y = torch.full((1, 3, 64, 128), 5.0, device=dev)
    p.forward(x, y, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    p.close()


def test_entry_refuses_bad_descriptors():
    """HAT_EINVAL / HAT_EUNSUPPORTED before any launch."""
    dev = _dev()
    from super_resolution_amd import ops
    pw, ln = _params(dev)
    x = torch.zeros(1, 3, 16, 16, device=dev)
    t, n = torch.zeros(1, 256, C, device=dev), torch.zeros(1, 256, C, dtype=torch.bfloat16, device=dev)
    gap = torch.zeros(1, ops.layernorm_blocks(), 16, device=dev)
    kw = dict(B=1, H=16, W=16, ldn=C, dtype=ops.HAT_BF16)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.head_fused(pw, x, None, t, n, ln[0], ln[1], **dict(kw, ldn=140))
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.head_fused(pw, x, None, t, n, ln[0], ln[1], gap=gap, gap_c=20, **kw)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.head_fused(pw, x, None, t.view(-1)[1:], n, ln[0], ln[1], **kw)        # t not 16-byte aligned
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.head_fused(pw, x, None, t, n, ln[0], ln[1], **dict(kw, dtype=ops.HAT_F32))
