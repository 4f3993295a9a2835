"""The exact-lattice method on the CPU (tests/lattice.py; the GPU half is test_gpu_lattice.py): every case of the tables is inside
the exact domain; on the lattice an fp32 accumulation in any order is bit-equal to fp64; and the method has teeth — structural
mutants of a 3 x 3 conv, the 13 x 13 conv and the folded ending (one weight element dropped or moved, a bias dropped, a clamped
border, a wrong border variant, a leaking pad channel) all fail `assert_bits` on lattice operands, while the same mutants on Gaussian
operands pass `helpers.check`'s bf16 bar: the gap the lattice tests close."""
import pytest
import torch
import torch.nn.functional as F

import lattice as L
from helpers import check, q, rnd
from super_resolution_amd import ops, packing
from super_resolution_amd._lib import HAT_BF16, HAT_F32


# ------------------------------------------------------------------------------------------------
# the domain conditions, for every case the GPU file launches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_conv_cases_are_inside_the_exact_domain(dtype):
    for k, cin, cout in L.CONV_PLAIN:
        for geom in L.GEOMS:
            L.conv_case(f"conv{k}.{cin}.{cout}.{geom}", geom, k, cin, cout, dtype)
    for f in L.CONV_FORMS:
        if dtype in f.dtypes:
            c = L.conv_case("form." + f.name, f.geom, f.k, f.cin, f.cout, dtype, f.opt)
            assert not f.opt.get("act") or float(c.ref.abs().max()) <= 4.0


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_linear_and_small_conv_cases_are_inside_the_exact_domain(dtype):
    for name, cin, cout in L.LIN_SHAPES:
        for geom in L.LIN_GEOMS:
            for form, opt in L.LIN_FORMS.items():
                if (form != "gelu" or dtype == "bf16") and dtype in L.lin_dtypes(cin, cout):
                    L.conv_case(f"lin.{name}.{geom}.{form}", geom, 1, cin, cout, dtype, opt)
    if dtype == "bf16":
        for form, opt in L.LIN_FP16.items():
            L.conv_case(f"lin.aggr144.{form}", (2, 19, 27), 1, 144, 144, "bf16", opt)
    for name, cin, cout in L.T3_SHAPES:
        for act in (0, 1, 2):
            if (act != 1 or dtype == "bf16") and dtype in L.t3_dtypes(cin, cout):
                L.conv_case(f"t3.{name}.{act}", L.T3_GEOM, 3, cin, cout, dtype, dict(colsum=True, act=act))


def test_bf16_only_kernels_cases_are_inside_the_exact_domain():
    for geom in L.AGGR_GEOMS:
        L.aggr_case(geom)
    for geom in L.ESC13_GEOMS:
        L.esc13_case(geom)
    for geom in L.SWEEP_GEOMS:
        for nout in (3, 1):
            L.sweep_case(geom, 64, nout, gelu=False)
        for C, mid in L.SQUEEZE_CM:
            c = L.sweep_case(geom, C, mid, gelu=True)
            assert float(c.ref.abs().max()) <= 4.0
    for shape in L.UPFOLD_SHAPES:
        L.upfold_case(shape)


def test_the_tables_cover_every_instantiation():
    """Every (nt, ceil(Cin / 32)) of hat_linear and every (nt, Cin_p) of hat_conv3x3_small gets a case, and every case runs on
    its own kernel (none falls back to hat_conv)."""
    assert {L.pw_pair(cin, cout, HAT_BF16) for _, cin, cout in L.LIN_SHAPES} == ops._PW_SHAPES
    assert {L.t3_pair(cin, cout) for _, cin, cout in L.T3_SHAPES} == ops._T3_SHAPES
    for _, cin, cout in L.LIN_SHAPES:
        assert "bf16" in L.lin_dtypes(cin, cout)
    for _, cin, cout in L.T3_SHAPES:
        assert "bf16" in L.t3_dtypes(cin, cout)
    assert {L.pw_pair(cin, cout, HAT_F32) for _, cin, cout in L.LIN_SHAPES if "f32" in L.lin_dtypes(cin, cout)} == {(9, 5), (12, 6), (4, 1), (4, 2)}
    # hat_conv64r: the same 64 -> 256 pixel-shuffle conv on the resident-weight kernel and, with a split source, just outside it
    forms = {f.name: f for f in L.CONV_FORMS}
    takes = lambda n, d: L.resident_kernel_takes(d, forms[n].k, forms[n].cin, forms[n].cout, forms[n].opt)
    assert takes("pixshuf2_resident", "bf16") and not takes("pixshuf2_generic", "bf16") and not takes("pixshuf2_resident", "f32")
    assert forms["pixshuf2_resident"].geom[2] % 16 == 0 and takes("pixshuf3", "bf16") and takes("lrelu_resident", "bf16")
    assert L.resident_kernel_takes("bf16", 3, 64, 64, None) and not L.resident_kernel_takes("bf16", 3, 64, 48, None)
    for C, mid in L.SQUEEZE_CM:
        assert all(ops.cab_squeeze_supported(C, mid, g[2], HAT_BF16) and ops.conv3x3_to_planes_supported(3, 64, g[2], HAT_BF16) for g in L.SWEEP_GEOMS)
    assert all(ops.upfold_supported(64, 3, 2, w, HAT_BF16) for _, w in L.UPFOLD_SHAPES)


def test_folded_ending_stays_on_the_lattice():
    """With wu, wl in {-2..2} every one of the twelve packed variants holds integers of at most 93 in magnitude at density 0.5 (234
    at density 1): exact in bf16; and the fold equals conv -> pixel_shuffle -> conv exactly in fp64."""
    for density, top in ((0.5, 93), (1.0, 234)):
        wu, bu, wl, bl = L.upfold_weights(f"fold{density}", density)
        G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
        for rs in range(4):
            for cs in range(3):
                Fv, bias = packing.upfold_variant(G, Bd, b0, rs, cs)
                assert torch.equal(Fv, Fv.round()) and float(Fv.abs().max()) <= top
                assert torch.equal(Fv.float().to(torch.bfloat16).double(), Fv) and torch.equal(bias, bias.round())
    c = L.upfold_case((3, 16))
    folded = packing.upfold_apply(c.x.permute(0, 3, 1, 2), *c.w) * c.out_scale + torch.tensor(c.mean, dtype=torch.float64)[None, :, None, None]
    assert torch.equal(folded, c.ref)


def test_a_case_outside_the_domain_raises():
    x = L.acts("dom.x", (1, 4, 4, 8))
    w = L.weights("dom.w", (8, 8, 3, 3))
    ok = dict(stored=[("x", x, torch.bfloat16), ("w", w, torch.bfloat16)], absum=L.conv_abs(x, w), unit=1.0, addends=[L.conv64(x, w)])
    L.assert_exact_domain("inside", **ok)
    with pytest.raises(AssertionError, match="does not survive"):
        L.assert_exact_domain("operand", **dict(ok, stored=[("x", x * 257.0, torch.bfloat16)]))
    with pytest.raises(AssertionError, match="off the result lattice"):
        L.assert_exact_domain("addend", **dict(ok, addends=[x * 0.3]))
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        L.assert_exact_domain("bound", **dict(ok, unit=2.0 ** -20))
    with pytest.raises(AssertionError, match="not exactly representable"):
        L.expect(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.bfloat16)


def test_expect_rounds_once_to_nearest_even_and_the_comparisons_report():
    v = torch.tensor([257.0, 259.0, 2049.0, 2051.0, -257.0, 0.375], dtype=torch.float64)
    assert L.expect(v, torch.bfloat16).tolist() == [256.0, 260.0, 2048.0, 2048.0, -256.0, 0.375]
    assert L.expect(v, torch.float16).tolist() == [257.0, 259.0, 2048.0, 2052.0, -257.0, 0.375]
    assert torch.equal(L.expect(v, torch.float32).double(), v)
    want = torch.zeros(2, 3, 4, 8)
    got = want.clone()
    L.assert_bits(got, want, "equal")
    got[1, 2, 3, 5], got[1, 0, 3, 5] = 1.0, 2.0
    with pytest.raises(AssertionError, match=r"2 of 192 elements differ.*\(b=1, y=0, x=3, c=5\): got 2.0 want 0.0"):
        L.assert_bits(got, want, "seam")
    with pytest.raises(AssertionError):
        L.assert_bits(torch.tensor([float("nan")]), torch.tensor([float("nan")]), "nan")
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        one = torch.tensor([1.0, -1.0, 0.0, 3.0], dtype=dt)
        up = torch.nextafter(one.float(), torch.tensor(9.0)).to(dt) if dt == torch.float32 else (one.view(torch.int16) + 1).view(dt)
        L.assert_ulp(up, one, "one ulp")
        with pytest.raises(AssertionError, match="more than 1 ulp"):
            L.assert_ulp(one * 1.25, one, "far")
    L.assert_ulp(torch.tensor([-0.0]), torch.tensor([0.0]), "signed zero")


# ------------------------------------------------------------------------------------------------
# order independence
# ------------------------------------------------------------------------------------------------
def test_fp32_accumulation_in_any_order_is_bit_equal_to_fp64():
    c = L.conv_case("order", (2, 19, 21), 3, 144, 144, "bf16", dict(out="f32", r1="f32"))
    x, w = c.x.float(), c.w.float()
    lib = F.conv2d(x.permute(0, 3, 1, 2), w, c.bias.float(), padding=1).permute(0, 2, 3, 1) + c.r1.float()
    L.assert_bits(lib, L.expect(c.ref, torch.float32), "torch's fp32 conv")
    # one fp32 add per (tap, channel block) in a shuffled order, the bias and the residual somewhere in the middle
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    terms = [(t, c0) for t in range(9) for c0 in range(0, C, 16)]
    order = torch.randperm(len(terms), generator=torch.Generator().manual_seed(5)).tolist()
    acc = torch.zeros(B, H, W, C)
    for n, i in enumerate(order):
        t, c0 = terms[i]
        acc = acc + xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W, c0:c0 + 16] @ w[:, c0:c0 + 16, t // 3, t % 3].t()
        if n == 17:
            acc = acc + c.r1.float()
        if n == 40:
            acc = acc + c.bias.float()
    L.assert_bits(acc, L.expect(c.ref, torch.float32), "a shuffled fp32 accumulation")
    # off the lattice the same two computations differ: the equality above is the lattice's doing
    xg, wg = rnd("og.x", (B, H, W, C)), rnd("og.w", (C, C, 3, 3), std=1 / 36)
    a = F.conv2d(xg.permute(0, 3, 1, 2), wg, padding=1).permute(0, 2, 3, 1)
    xq = F.pad(xg, (0, 0, 1, 1, 1, 1))
    b = torch.zeros(B, H, W, C)
    for i in order:
        t, c0 = terms[i]
        b = b + xq[:, t // 3:t // 3 + H, t % 3:t % 3 + W, c0:c0 + 16] @ wg[:, c0:c0 + 16, t // 3, t % 3].t()
    assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# mutation sensitivity
# ------------------------------------------------------------------------------------------------
def _typical(t):
    """Index of a typical element: the nonzero one of median magnitude (the first of them)."""
    idx = t.nonzero()
    mag = t[tuple(idx.t())].abs()
    return tuple(int(v) for v in idx[int(torch.argsort(mag, stable=True)[len(mag) // 2])])


def _conv_mutants(k):
    """name -> f(x (B,H,W,Cin), w (Cout,Cin,k,k), bias) -> (B,H,W,Cout) fp64: a conv that is wrong in one structural detail, each
    confined to what a real indexing slip touches and small enough that the Gaussian bar lets it through."""
    h = k // 2

    def tap_zeroed(x, w, b):            # one (output row, channel, tap) of the packed matrix reads zero
        w = w.clone()
        w[(5,) + _typical(w[5])] = 0
        return L.conv64(x, w, b)

    def tap_moved(x, w, b):             # ... or lands on the neighbouring tap
        w = w.clone()
        ci, ty, tx = _typical(w[7, :, :, :k - 1])
        w[7, ci, ty, tx + 1] += w[7, ci, ty, tx]
        w[7, ci, ty, tx] = 0
        return L.conv64(x, w, b)

    def bias_dropped(x, w, b):
        b = b.clone()
        b[_typical(b)] = 0
        return L.conv64(x, w, b)

    def clamp_edge(x, w, b):            # the first column right of sample 0's image repeats the last one instead of zero, in one channel
        xp = F.pad(x.double().permute(0, 3, 1, 2), (h, h, h, h))        # (13 x 13: 13 taps of 16 channels see it, so beside ONE typical pixel)
        if k == 3:
            xp[0, 3, h:-h, -h] = x[0, :, -1, 3].double()
        else:
            y = _typical(x[0, :, -1, 3])[0]
            xp[0, 3, h + y, -h] = x[0, y, -1, 3].double()
        return F.conv2d(xp, w.double(), b.double()).permute(0, 2, 3, 1)

    def pad_leak(x, w, b):              # the last ragged tile's columns read one pad channel (the poison) under one weight element
        y = L.conv64(x, w, b)
        co = 9
        elem = w[(co,) + _typical(w[co])].double()
        y[:, :, (16 if k == 3 else -2):, co] += L.POISON * elem       # (one of 16 channels weighs more: the last two columns there)
        return y

    m = dict(tap_zeroed=tap_zeroed, tap_moved=tap_moved, bias_dropped=bias_dropped, clamp_edge=clamp_edge, pad_leak=pad_leak)
    if k == 13:
        del m["bias_dropped"]       # (hat_esc_conv13 has no bias; over 16 channels a dropped one is 2.4 % and the Gaussian bar sees it)
    return m


def _gaussian_conv(k, cin, cout, geom):
    x = q(rnd(f"mg{k}.x", geom + (cin,)), "bf16")
    w = q(rnd(f"mg{k}.w", (cout, cin, k, k), std=(cin * k * k) ** -0.5), "bf16")
    return x, w, rnd(f"mg{k}.b", (cout,), std=0.1)


@pytest.mark.parametrize("k,cin,cout", [(3, 144, 144), (13, 16, 16)], ids=["conv3x3_144", "conv13x13_16"])
def test_conv_mutants_fail_on_the_lattice_and_pass_the_gaussian_bar(k, cin, cout):
    geom = (2, 19, 21)
    c = L.conv_case(f"mut{k}", geom, k, cin, cout, "bf16")
    gx, gw, gb = _gaussian_conv(k, cin, cout, geom)
    gref = q(L.conv64(gx, gw, gb).float(), "bf16").double()
    for name, f in _conv_mutants(k).items():
        mut = f(c.x, c.w, c.bias)
        for tdt in (torch.float32, torch.bfloat16):
            with pytest.raises(AssertionError, match="elements differ"):
                L.assert_bits(L.expect(mut, tdt), L.expect(c.ref, tdt), name)
        check(q(f(gx, gw, gb).float(), "bf16").double(), gref, "bf16", f"{name} on Gaussian operands")     # the gap: it passes
    L.assert_bits(L.expect(L.conv64(c.x, c.w, c.bias), torch.bfloat16), L.expect(c.ref, torch.bfloat16), "the unmutated conv")


def _upfold_mutants():
    """name -> f(x (B,H,W,64), wu, bu, wl, bl) -> (B,3,2H,2W) fp64 before out_scale / mean."""
    def three(x, wu, bu, wl, bl):
        return L.conv64(L.pixel_shuffle_last(L.conv64(x, wu, bu), 2), wl, bl).permute(0, 3, 1, 2)

    def tap_zeroed(x, wu, bu, wl, bl):
        wu = wu.clone()
        wu[(5,) + _typical(wu[5])] = 0
        return three(x, wu, bu, wl, bl)

    def tap_moved(x, wu, bu, wl, bl):
        wu = wu.clone()
        ci, ty, tx = _typical(wu[9, :, :, :2])
        wu[9, ci, ty, tx + 1] += wu[9, ci, ty, tx]
        wu[9, ci, ty, tx] = 0
        return three(x, wu, bu, wl, bl)

    def bias_dropped(x, wu, bu, wl, bl):
        bu = bu.clone()
        bu[_typical(bu)] = 0
        return three(x, wu, bu, wl, bl)

    def interior_bias_on_the_corners(x, wu, bu, wl, bl):    # the four corner pixels take the interior variant's folded bias
        G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
        y = three(x, wu, bu, wl, bl)
        H, W = x.shape[1:3]
        py, px = torch.arange(H)[:, None], torch.arange(W)[None, :]
        rs, cs = (py == 0) * 1 + (py == H - 1) * 2, (px == 0) * 1 + (px == W - 1) * 2
        inner = packing.upfold_variant(G, Bd, b0, 0, 0)[1]
        for r in range(4):
            for s in range(4):
                if r and s:
                    d = F.pixel_shuffle(((inner - packing.upfold_variant(G, Bd, b0, r, s)[1]).reshape(12, 1, 1) * ((rs == r) & (cs == s)))[None], 2)
                    y = y + d
        return y

    def clamp_edge(x, wu, bu, wl, bl):      # the halo right of one typical edge pixel of sample 0 repeats it instead of zero, in one channel
        xp = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1))        # (a whole clamped column is 0.15 at its worst: the Gaussian bar's 0.14 sees it)
        y = _typical(x[0, :, -1, 3])[0]
        xp[0, 3, 1 + y, -1] = x[0, y, -1, 3].double()
        y1 = F.conv2d(xp, wu.double(), bu.double()).permute(0, 2, 3, 1)
        return L.conv64(L.pixel_shuffle_last(y1, 2), wl, bl).permute(0, 3, 1, 2)

    def pad_leak(x, wu, bu, wl, bl):        # the last column of one plane reads a pad channel of the 72-wide rows under one folded weight
        G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
        Fv = packing.upfold_variant(G, Bd, b0, 0, 0)[0][1, 0, 0]            # (64, 5, 5) of colour 1, sub-pixel (0, 0)
        y = three(x, wu, bu, wl, bl).clone()
        y[:, 1, :, -1:] += L.POISON * Fv[_typical(Fv)]          # (two columns of the three planes are 1.4 %: the Gaussian bar sees that)
        return y

    return dict(tap_zeroed=tap_zeroed, tap_moved=tap_moved, bias_dropped=bias_dropped, interior_bias_on_the_corners=interior_bias_on_the_corners,
                clamp_edge=clamp_edge, pad_leak=pad_leak)


def _interior_variant_everywhere(x, wu, bu, wl, bl):
    G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
    Fv, bias = packing.upfold_variant(G, Bd, b0, 0, 0)
    return F.pixel_shuffle(F.conv2d(x.double().permute(0, 3, 1, 2), Fv.reshape(12, 64, 5, 5), bias.reshape(-1), padding=2), 2)


def test_upfold_mutants_fail_on_the_lattice_and_pass_the_gaussian_bar():
    c = L.upfold_case((11, 32))
    ref = (c.ref - torch.tensor(c.mean, dtype=torch.float64)[None, :, None, None]) / c.out_scale
    g = torch.Generator().manual_seed(119)          # test_gpu_upfold.py's layer
    gx = torch.randn(2, 11, 32, 64, generator=g).to(torch.bfloat16).double()
    gw = (torch.randn(256, 64, 3, 3, generator=g) / 24.0, torch.randn(256, generator=g) * 0.1,
          torch.randn(3, 64, 3, 3, generator=g) * (0.6 / 24.0), torch.randn(3, generator=g) * 0.1)
    gw = tuple(t.double() for t in gw)
    ring = L.ring_mask(22, 64)
    gref = L.conv64(L.pixel_shuffle_last(L.conv64(gx, gw[0], gw[1]), 2), gw[2], gw[3]).permute(0, 3, 1, 2)
    for name, f in _upfold_mutants().items():
        mut = f(c.x, *c.w)
        with pytest.raises(AssertionError, match="elements differ"):
            L.assert_bits(L.expect(mut, torch.float32), L.expect(ref, torch.float32), name)
        check(f(gx, *gw), gref, "bf16", f"{name} on Gaussian operands")
    # the whole interior variant on the ring: the lattice sees it on the ring and nowhere else.  (This one is as large as the
    # values there, and the Gaussian bar sees it as well; the bias part on the corners, above, it does not.)
    mut = _interior_variant_everywhere(c.x, *c.w)
    assert torch.equal(mut[..., ~ring], ref[..., ~ring]) and not torch.equal(mut[..., ring], ref[..., ring])
    with pytest.raises(AssertionError, match="elements differ"):
        L.assert_bits(L.expect(mut, torch.float32), L.expect(ref, torch.float32), "interior variant everywhere")
