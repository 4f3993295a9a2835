"""Host-side checks of the structural probes (tests/probes.py; DESIGN "Structural probes"): the selector weights survive the
packers' roundings, the fp64 restatement is the oracle's gated FFN, the emulated storage roundings stay inside the bars for every
shape and shift test_gpu_probes.py launches (no element excluded) and the bars are four times them, every mutant leaves the bar by a
factor of four, two of the mutants pass the tolerance bars of test_hab_tail_fused on its dense weights, and the shift sets reach every
weight position.  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lattice as L
import probes as P
from helpers import check, q, rnd

KEYS = [("v2", 144), ("v3", 144), ("v3", 180)]
_ID = lambda k: f"{k[0]}-{k[1]}"


def _tB(C, geom):
    B, H, W = geom
    return P.stage0_case(C, geom).ref.reshape(B, H * W, C)


@pytest.mark.parametrize("C", [144, 180])
def test_selector_weights_are_exact_in_storage(C):
    """The gamma fold and the beta fold are bf16-exact, every depthwise / fc2 value fp16-exact, at every shift; a unit and its gate
    unit never share a tap; each fc1 row has DENSITY weights, each unit one tap, each fc2 column one weight."""
    hid = P.HID[C]
    for s in P.covering_shifts(C):
        sd = P.selector_ffn(C, s)
        P.assert_selector_domain(sd, C)
        Wd = sd["m.dw.weight"].reshape(2 * hid, 9)
        assert torch.all((sd["m.fc1.weight"] != 0).sum(1) == P.DENSITY) and torch.all((Wd != 0).sum(1) == 1)
        assert torch.all((sd["m.fc2.weight"] != 0).sum(0) == 1)
        assert torch.all(Wd[:hid].abs().argmax(1) != Wd[hid:].abs().argmax(1))
        assert torch.all(sd["m.fc1.bias"][1:] != sd["m.fc1.bias"][:-1]) and torch.all(sd["m.dw.bias"][1:hid] != sd["m.dw.bias"][:hid - 1])


@pytest.mark.parametrize("C", [144, 180])
def test_stage0_cases_are_on_the_lattice(C):
    """stage0_case raises outside the exact domain; tB is an fp32 number; at 144 the stream survives FP16 rows; B = 2 has per-sample
    operands that differ."""
    for geom in P.SHAPES:
        c = P.stage0_case(C, geom)
        assert torch.equal(c.ref.float().double(), c.ref)
        if C == 144:
            P.stage0_fp16_ok(c)
            if geom[0] == 2:
                assert not torch.equal(c.wf[0], c.wf[1]) and not torch.equal(c.bias_b[0], c.bias_b[1])
        L.expect(c.ref + P.selector_ffn(C, 3)["m.fc2.bias"], torch.float32)


@pytest.mark.parametrize("C", [144, 180])
def test_restatement_is_the_oracle(C):
    geom = (2, 9, 17)
    sd = P.selector_ffn(C, 5)
    tB = _tB(C, geom)
    ref = P.reference_update(tB, sd, geom[1:])
    assert float((P.tail_update(tB, sd, geom[1:]) - ref).abs().max()) <= 1e-11 * float(ref.abs().max())


def _probes_of(key):
    """(kernel generation, C) -> the (geom, shift) pairs test_gpu_probes.py launches on it."""
    gen, C = key
    out = [(g, s) for g in P.SHAPES for s in P.few_shifts(C)]
    if gen == "v3":
        out += [(P.FULL_SHAPE, s) for s in P.covering_shifts(C) if s not in P.few_shifts(C)]
    return out


@functools.lru_cache(maxsize=None)
def _emulated_worst(key):
    gen, C = key
    worst = 0.0
    for geom, s in _probes_of(key):
        sd = P.selector_ffn(C, s)
        tB = _tB(C, geom)
        ref = P.reference_update(tB, sd, geom[1:])
        worst = max(worst, P.worst_ratio(P.tail_update(tB, sd, geom[1:], gen), ref, 1.0)[0])
    return worst


@pytest.mark.parametrize("key", KEYS, ids=_ID)
def test_bars_are_four_times_the_emulated_roundings(key):
    """Over every probe the GPU tests launch and every element: the emulation of the documented roundings stays within tau (|ref| +
    1) / 4, and tau is no looser than twice that rule."""
    worst = _emulated_worst(key)
    print(f"{key}: max |emulation - reference| / (|reference| + 1) = {worst:.4f}, tau = {P.TAU[key]}")
    assert 4.0 * worst <= P.TAU[key] <= 8.0 * worst, (key, worst, P.TAU[key])


@pytest.mark.parametrize("slip", P.SLIPS)
@pytest.mark.parametrize("key", KEYS, ids=_ID)
def test_mutants_leave_the_bar(key, slip):
    """One slip on one hidden unit (with the kernel's roundings emulated on top) moves at least one element of the update beyond FOUR
    times the bar, on a shape and shift the GPU tests launch."""
    gen, C = key
    geom, s, unit = P.MUTANTS[key][slip]
    assert (geom, s) in _probes_of(key)
    sd = P.selector_ffn(C, s)
    tB = _tB(C, geom)
    ref = P.reference_update(tB, sd, geom[1:])
    ratio, at = P.worst_ratio(P.tail_update(tB, sd, geom[1:], gen, slip, unit), ref, P.TAU[key])
    assert ratio > 4.0, f"{key} {slip} on unit {unit}: worst element {at} is only {ratio:.2f} x the bar"
    with pytest.raises(AssertionError):
        P.assert_update(P.tail_update(tB, sd, geom[1:], gen, slip, unit), ref, P.TAU[key], "mutant", geom)


@pytest.mark.parametrize("slip", ["dw_bias_dropped", "corner_clamped"])
def test_dense_weights_let_these_mutants_through(slip):
    """Documentation: on the dense Gaussian weights of test_gpu_ops.py::test_hab_tail_fused the same slips pass helpers.check and the
    1.2e-2 relative-L2 bar on the update, with the kernel's roundings emulated on top."""
    B, H, W = 1, 19, 27
    C, mid, hid = 144, 6, 288
    n, y16 = q(rnd("htn", (B, H, W, C)), "bf16"), q(rnd("hty", (B, H, W, 16)), "bf16")
    c1 = q(F.gelu(rnd("htc1", (B, H, W, mid))), "bf16")
    t = rnd("htt", (B, H, W, C), std=1.5) + 0.3
    wa, ba = q(rnd("htwa", (C, C), std=C ** -0.5), "bf16"), rnd("htba", (C,), std=0.1)
    w2, b2c, wk = rnd("htw2", (C, mid, 3, 3), std=(9 * mid) ** -0.5), rnd("htb2", (C,), std=0.1), rnd("htwk", (5,), std=1.0)
    sd = {
        "n2.weight": 1 + rnd("fg", (C,), std=0.1), "n2.bias": rnd("fbb", (C,), std=0.1),
        "m.fc1.weight": q(rnd("f1w", (2 * hid, C), std=C ** -0.5), "bf16"), "m.fc1.bias": rnd("f1b", (2 * hid,), std=0.1),
        "m.dw.weight": rnd("fdw", (2 * hid, 1, 3, 3), std=1 / 3).half().float(), "m.dw.bias": rnd("fdb", (2 * hid,), std=0.1).half().float(),
        "m.fc2.weight": rnd("f2w", (C, hid), std=hid ** -0.5).half().float(), "m.fc2.bias": rnd("f2b", (C,), std=0.1),
    }
    sd = {k: v.double() for k, v in sd.items()}
    c2 = F.conv2d(c1.permute(0, 3, 1, 2).double(), w2.double(), b2c.double(), padding=1)
    e = torch.sigmoid(F.conv1d(c2.mean((2, 3))[:, None, :], wk.double()[None, None, :], padding=2))[:, 0]
    xin = torch.cat([y16, n[..., 16:]], -1)
    tb = (t.double() + F.linear(xin.double(), wa.double(), ba.double()) + 0.37 * (e[:, :, None, None] * c2).permute(0, 2, 3, 1)).reshape(B, H * W, C)
    upd_ref = P.reference_update(tb, sd, (H, W))
    upd = P.tail_update(tb, sd, (H, W), "v3", slip, 37)
    assert float((upd - P.tail_update(tb, sd, (H, W), "v3")).abs().max()) > 0       # the slip did change something
    rel = float((upd - upd_ref).norm() / upd_ref.norm())
    assert rel <= 1.2e-2, rel
    check(tb + upd, tb + upd_ref, "bf16", "mutant under the tolerance bars")


@pytest.mark.parametrize("C", [144, 180])
def test_shift_sets_reach_every_weight_position(C):
    """Across the covering shift set every fc1 (unit, channel) pair, every fc2 (channel, unit) pair and every (unit, tap) pair is
    non-zero in at least one probe; the few-shift set already puts an fc1 weight into every k-step of every row's fragment tile
    (channels >= 128 included) for some unit."""
    hid = P.HID[C]
    fc1, fc2, taps = torch.zeros(2 * hid, C, dtype=torch.bool), torch.zeros(C, hid, dtype=torch.bool), torch.zeros(2 * hid, 9, dtype=torch.bool)
    for s in P.covering_shifts(C):
        sd = P.selector_ffn(C, s)
        fc1 |= sd["m.fc1.weight"] != 0
        fc2 |= sd["m.fc2.weight"] != 0
        taps |= sd["m.dw.weight"].reshape(2 * hid, 9) != 0
    assert fc1.all() and fc2.all() and taps.all()
    few = torch.zeros(2 * hid, C, dtype=torch.bool)
    for s in P.few_shifts(C):
        few |= P.selector_ffn(C, s)["m.fc1.weight"] != 0
    assert few[:, 128:].any()


def test_ocab_cases():
    """hat_ocab_qkv: the cases are inside the exact domain and every (n-tile, k-step) fragment of the stacked weight holds a weight,
    the 16-deep half step included.  hat_ocab_mlp: |S| <= 4, r1 survives FP16, the fc2 selectors are powers of two, one per column,
    and the shift set routes a value through every (n-tile, k-step) fragment of fc2 — also (8, 5..8), which live in registers."""
    for npix in P.QKV_NPIX:
        c = P.qkv_case(npix)
        L.expect(c.ref, torch.bfloat16)
    assert P.qkv_fragments_hit(c).all()
    m = P.mlp_case()
    assert float(m.S.abs().max()) <= 4.0 and float(m.S.abs().max()) > 2.0
    for s in P.MLP_SHIFTS:
        W2 = P.mlp_fc2(s)
        nz = W2[W2 != 0].abs()
        assert torch.all((W2 != 0).sum(0) == 1) and torch.equal(torch.log2(nz), torch.log2(nz).round())
        assert torch.equal(W2.to(torch.bfloat16).double(), W2)
        lo, hi = P.mlp_expect(m, W2)
        assert torch.all(hi >= lo) and float((hi - lo).max()) < 0.07          # a band of two bf16 ulps of O(1) values, not a tolerance
    assert P.mlp_fragments_hit(P.MLP_SHIFTS).all()
    assert not P.mlp_fragments_hit(P.MLP_SHIFTS[:1]).all()


def test_mlp_band_catches_a_misrouted_column():
    """One fc2 weight read from the neighbouring column leaves the one-ulp band."""
    m = P.mlp_case()
    W2 = P.mlp_fc2(17)
    lo, hi = P.mlp_expect(m, W2)
    h = P.r_bf16(L.act64(m.S, 1))
    good = (m.r1 + m.b2 + h @ W2.t()).float()
    P.assert_band(good, lo, hi, "the expectation itself")
    bad = W2.clone()
    bad[:, [200, 201]] = W2[:, [201, 200]]
    with pytest.raises(AssertionError):
        P.assert_band((m.r1 + m.b2 + h @ bad.t()).float(), lo, hi, "misrouted")
