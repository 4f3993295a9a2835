"""Structural probes (DESIGN "Structural probes"): the gated FFN of the HAB tail is not linear, so it cannot sit on the exact
lattice (tests/lattice.py) — but its WEIGHTS can be chosen so that every output element depends on a handful of identifiable
inputs: a selector fc1 (a few +-1, +-1/2 per row), ONE depthwise tap per hidden unit, ONE fc2 weight per hidden unit.  A structural
slip (a tap, a halo pixel, a bias, a k-slot, a routed column) then moves an output element by O(1) where the kernels' bf16 / fp16
rounding moves it by O(0.01), and each element is judged on its own:  |got - ref| <= tau (|ref| + 1)  on the FFN update.
Stage 0 of the tail kernels is linear and runs on the lattice, so tB is exact and the update can be isolated exactly.

Host only.  Here: the selector weights, the stage-0 lattice operands (lattice.py's draws and domain check), an fp64 restatement of
the tail that can emulate the kernels' documented storage roundings and carry one slip (the mutants), the bars tau, the
hat_ocab_qkv / hat_ocab_mlp cases, and the case tables that test_gpu_probes.py launches and test_probes_cpu.py checks."""
import functools

import torch
import torch.nn.functional as F

import lattice as L
from oracle import hat_oracle as O

SHAPES = [(1, 8, 16), (1, 16, 32), (1, 24, 48), (1, 9, 17), (1, 3, 5), (2, 9, 17)]     # (B, H, W); tiles are 8 rows x 16 columns
FULL_SHAPE = (1, 16, 32)          # where the covering shift set runs
DENSITY = 4                       # non-zeros of an fc1 row
HID = {144: 288, 180: 360}
GATE_OFFSET = 7                   # the gate rows of fc1 start 7 channels further on: a unit and its gate unit see different rows


def few_shifts(C: int):
    return [0, 5, C - 1]


def covering_shifts(C: int):
    """One fc2 weight per hidden unit reaches a (channel, unit) pair in one probe only, so every pair needs C probes; the fc1
    pairs (C / DENSITY shifts) and the taps (9 shifts) are covered several times over by them."""
    return list(range(C))


# ------------------------------------------------------------------------------------------------
# the bars.  tau = 4 x max over every shape and shift the GPU tests use, and every element, of |emulation - reference| / (|reference|
# + 1), rounded up to two digits (test_probes_cpu.py recomputes the maxima and holds these constants to 4 x .. 8 x of them).
# Nothing here comes from a kernel's output.  Keys: (generation, embed_dim).
# ------------------------------------------------------------------------------------------------
TAU = {("v2", 144): 0.22, ("v3", 144): 0.25, ("v3", 180): 0.33}


# ------------------------------------------------------------------------------------------------
# selector weights
# ------------------------------------------------------------------------------------------------
_V4 = (1.0, -0.5, 0.5, -1.0)
_F2 = (2.0, -1.0, 1.0, -2.0)


def selector_ffn(C: int, s: int, d: int = DENSITY, zero_fc2: bool = False):
    """State dict (fp64) of LayerNorm2 ("n2") + GatedDconvFFN ("m") + the next LayerNorm ("n1") of one probe: shift s, density d.
    fc1 row j: the four values of _V4 (rotated by j) at channels (j + s + i C / d) mod C, gate rows GATE_OFFSET further on; its
    bias small dyadic numbers that differ between neighbours.  Depthwise: unit j of the a half has ONE tap, (j + s) mod 9, its gate
    unit (j + s + 4) mod 9.  fc2: column k has ONE weight, at channel (k + s) mod C.  gamma a power of two, beta dyadic: the
    third generation's fold (W1 diag gamma, W1 beta + b1 as a bf16 k-slot) is exact."""
    hid = HID[C]
    j = torch.arange(2 * hid)
    gate = (j >= hid).long()
    W1 = torch.zeros(2 * hid, C, dtype=torch.float64)
    v4 = torch.tensor(_V4, dtype=torch.float64)
    for i in range(d):
        W1[j, (j + s + GATE_OFFSET * gate + i * (C // d)) % C] = v4[(j + i) % 4]
    b1 = ((3 * j) % 11 - 5).double() / 16
    u = j % hid                                                      # the unit's index within its half
    tap = (u + s + 4 * gate) % 9
    Wd = torch.zeros(2 * hid, 9, dtype=torch.float64)
    Wd[j, tap] = v4[(u + gate) % 4]
    bd = torch.where(gate == 0, (5 * u) % 13 - 6, (7 * u) % 11 - 5).double() / 8
    k = torch.arange(hid)
    W2 = torch.zeros(C, hid, dtype=torch.float64)
    if not zero_fc2:
        W2[(k + s) % C, k] = torch.tensor(_F2, dtype=torch.float64)[(k + k // C) % 4]
    c = torch.arange(C)
    return {"n2.weight": 2.0 ** ((c % 3) - 1).double(), "n2.bias": ((5 * c) % 7 - 3).double() / 8,
            "m.fc1.weight": W1, "m.fc1.bias": b1, "m.dw.weight": Wd.reshape(2 * hid, 1, 3, 3), "m.dw.bias": bd,
            "m.fc2.weight": W2, "m.fc2.bias": ((3 * c) % 17 - 8).double() / 4,
            "n1.weight": 1.0 + ((7 * c) % 5 - 2).double() / 16, "n1.bias": ((3 * c) % 5 - 2).double() / 8}


def assert_selector_domain(sd, C: int):
    """What the packers round must survive it: W1, W1 diag(gamma) and W1 beta + b1 in bf16 (hat_ffn2 rounds the first, pack_ffn3 the
    other two), the depthwise taps and bias and fc2 in fp16."""
    W1, b1, g_, b_ = sd["m.fc1.weight"], sd["m.fc1.bias"], sd["n2.weight"], sd["n2.bias"]
    bf, hf = torch.bfloat16, torch.float16
    L.assert_exact_domain(f"selector weights, C = {C}", absum=1.0, unit=1.0,
                          stored=[("W1", W1, bf), ("W1 gamma", W1 * g_[None, :], bf), ("W1 beta + b1", W1 @ b_ + b1, bf),
                                  ("dw", sd["m.dw.weight"], hf), ("dw bias", sd["m.dw.bias"], hf), ("fc2", sd["m.fc2.weight"], hf),
                                  ("b1", b1, torch.float32), ("b2", sd["m.fc2.bias"], torch.float32)])
    assert torch.equal(torch.log2(g_), torch.log2(g_).round()), "gamma is a power of two"


# ------------------------------------------------------------------------------------------------
# stage 0 on the lattice
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage0_case(C: int, geom) -> L.Case:
    """The operands of the tail kernels' fused stage 0 and the exact tB (`ref`, (B, H, W, C)).  144: lattice.aggr_case (x is the
    LayerNorm1 rows n, x0 the 16-channel y16, r1 the stream t).  180: tB = t + W_aggr . [y16 | n[16:]] + r2scale * c2 + bias, r2scale
    per sample."""
    if C == 144:
        c = L.aggr_case(geom)
        c.n, c.y16, c.t = c.x, c.x0, c.r1
        return c
    B, H, W = geom
    key = f"stage0_180{geom}"
    c = L.Case(geom=geom, C=C)
    c.n, c.y16 = L.acts(key + ".n", (B, H, W, C)), L.acts(key + ".y", (B, H, W, 16))
    c.c2 = L.acts(key + ".c2", (B, H, W, C), 1)
    c.r2scale = L.draw(key + ".sc", (B, C), 6, 2)
    c.wa = L.weights(key + ".wa", (C, C))
    c.bias = L.draw(key + ".b", (C,), 8, 2)
    c.t = L.draw(key + ".t", (B, H, W, C), 64, 2)
    assert B == 1 or not torch.equal(c.r2scale[0], c.r2scale[-1])
    xin = torch.cat([c.y16, c.n[..., 16:]], -1)
    term = c.r2scale[:, None, None, :] * c.c2
    c.ref = c.t + L.conv64(xin, c.wa[:, :, None, None]) + term + c.bias
    absum = c.t.abs() + L.conv_abs(xin, c.wa[:, :, None, None]) + term.abs() + c.bias.abs()
    bf = torch.bfloat16
    L.assert_exact_domain(key, stored=[("n", c.n, bf), ("y16", c.y16, bf), ("c2", c.c2, bf), ("wa", c.wa, bf), ("r2scale", c.r2scale, torch.float32),
                                       ("bias", c.bias, torch.float32), ("t", c.t, torch.float32)],
                          absum=absum, unit=0.125, addends=[c.t, c.bias, term, c.ref])
    return c


def stage0_fp16_ok(c: L.Case):
    """The stream t of the case survives FP16 rows (the FP16-in launches read the same numbers)."""
    L.assert_exact_domain("t as FP16 rows", stored=[("t", c.t, torch.float16)], absum=1.0, unit=1.0)


# ------------------------------------------------------------------------------------------------
# the tail in fp64: reference, emulation of the documented roundings, one slip
# ------------------------------------------------------------------------------------------------
def r_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def r_f16(x):
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def r_f16_rtz(x):
    """fp32 -> fp16 toward zero (v_cvt_pkrtz_f16_f32: how the kernels store U)."""
    v = x.to(torch.float32)
    h = v.to(torch.float16)
    over = h.to(torch.float32).abs() > v.abs()
    return torch.where(over, h.view(torch.int16) - 1, h.view(torch.int16)).view(torch.float16).to(torch.float64)


_ID = lambda x: x
SLIPS = ["tap_moved", "swap_a_gate", "dw_bias_dropped", "halo_is_bias", "seam_is_border", "fc1_high_channel_dropped", "fc2_moved",
         "corner_clamped"]


def reference_update(tB, sd, hw):
    """The fp64 reference of the FFN update t_out - tB: the oracle's own functions on the probe's weights."""
    return O.gated_dconv_ffn(O._ln(tB, sd, "n2"), hw, sd, "m")


def tail_update(tB, sd, hw, gen=None, slip=None, unit=0):
    """t_out - tB = fc2(a * SiLU(g)) + b2, [a | g] = dwconv3x3(fc1(LayerNorm2(tB))), tB (B, N, C) fp64, restated step by step.

    gen None: plain fp64 (test_probes_cpu.py pins it to reference_update).  gen "v2" / "v3": the storage roundings the kernel
    headers document — hat_ffn2.hip: LayerNorm2's output and W1 to bf16, the fc1 bias an fp32 addend; hat_tail3.hip / hat_tail3l.hip:
    xhat, W1 diag(gamma) and the k-slot W1 beta + b1 to bf16; both: U to fp16 toward zero, zero outside the image, one fp16 rounding per
    depthwise tap (v_pk_fma_f16 on an accumulator that starts as the bias), hat_gated_ffn.h's gate in packed fp16 step by step (the
    fp16 constant -log2 e, exp2, + 1, rcp, g * r, a * (g * r)), fp16 operands of fc2 — with everything accumulated in fp32 done in
    fp64 and exp2 / rcp exact before their rounding.

    slip: one of SLIPS on hidden unit `unit` of the a half (or the fc1 row `unit` for the fc1 slip): a mutant."""
    H, W = hw
    B, N, C = tB.shape
    g_, b_ = sd["n2.weight"], sd["n2.bias"]
    W1, b1 = sd["m.fc1.weight"], sd["m.fc1.bias"]
    Wd, bd = sd["m.dw.weight"].reshape(-1, 9).clone(), sd["m.dw.bias"].clone()
    W2, b2 = sd["m.fc2.weight"].clone(), sd["m.fc2.bias"]
    hid = W2.shape[1]
    rb, rh, rz = (r_bf16, r_f16, r_f16_rtz) if gen else (_ID, _ID, _ID)
    W1w = W1
    if slip == "fc1_high_channel_dropped":
        hi = (W1[unit, 128:] != 0).nonzero()
        assert hi.numel(), "the unit has no fc1 weight at a channel >= 128"
        W1w = W1.clone()
        W1w[unit, 128 + int(hi[-1])] = 0
    mu = tB.mean(-1, keepdim=True)
    xh = (tB - mu) / torch.sqrt(((tB - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    if gen == "v3":
        bk = rb(W1 @ b_ + b1)
        u = rz(rb(xh) @ rb(W1w * g_[None, :]).t() + bk)
    else:
        bk = b1
        u = rz(rb(xh * g_ + b_) @ rb(W1w).t() + bk)
    U = u.reshape(B, H, W, 2 * hid)
    Up = F.pad(U, (0, 0, 1, 1, 1, 1))
    if slip == "halo_is_bias":
        outside = torch.ones(H + 2, W + 2, dtype=torch.bool)
        outside[1:-1, 1:-1] = False
        Up[:, :, :, unit] = torch.where(outside, bk[unit], Up[:, :, :, unit])
    if slip == "corner_clamped":
        Up[:, 0, 0, unit] = U[:, 0, 0, unit]
    if slip == "tap_moved":
        Wd[unit] = torch.roll(Wd[unit], 1)
    if slip == "dw_bias_dropped":
        bd[unit] = 0
    acc = bd.expand(B, H, W, 2 * hid).clone()
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for t in range(9):
        ty, tx = divmod(t, 3)
        term = Up[:, ty:ty + H, tx:tx + W, :] * Wd[:, t]
        if slip == "seam_is_border":          # the neighbour across x = 16 or y = 8 reads as zero
            dead = ((xs == 15) if tx == 2 else (xs == 16) if tx == 0 else (xs < 0)) | ((ys == 7) if ty == 2 else (ys == 8) if ty == 0 else (ys < 0))
            term = term.clone()
            term[..., unit] = torch.where(dead, 0.0, term[..., unit])
        acc = rh(acc + term)
    a, g = acc[..., :hid].clone(), acc[..., hid:].clone()
    if slip == "swap_a_gate":
        a[..., unit], g[..., unit] = acc[..., hid + unit], acc[..., unit]
    if gen:
        e1 = rh(rh(torch.exp2(rh(g * r_f16(torch.tensor(-1.4426950408889634, dtype=torch.float64))))) + 1.0)
        p = rh(a * rh(g * rh(1.0 / e1)))
    else:
        p = a * g * torch.sigmoid(g)
    if slip == "fc2_moved":
        c = int((W2[:, unit] != 0).nonzero()[0])
        v = W2[c, unit].clone()
        W2[c, unit] = 0
        W2[(c + 1) % C, unit] = v
    return p.reshape(B, N, hid) @ W2.t() + b2


# One (shape, shift, hidden unit) per slip and kernel at which the mutant moves some element of the update beyond 4 tau (|ref| + 1): the
# shapes and shifts are among those the GPU tests launch.  The single-pixel slips (a corner, a border ring under one small bias) are
# visible on the units whose U and gate are not small there; these are such units (found by scanning the fp64 restatement).
_BIG = (1, 16, 32)
MUTANTS = {
    ("v2", 144): {"tap_moved": (_BIG, 0, 40), "swap_a_gate": (_BIG, 143, 80), "dw_bias_dropped": (_BIG, 143, 80), "halo_is_bias": (_BIG, 5, 40),
                  "seam_is_border": (_BIG, 5, 135), "fc1_high_channel_dropped": (_BIG, 5, 135), "fc2_moved": (_BIG, 0, 40),
                  "corner_clamped": ((2, 9, 17), 143, 163)},
    ("v3", 144): {"tap_moved": (_BIG, 0, 40), "swap_a_gate": (_BIG, 143, 80), "dw_bias_dropped": (_BIG, 143, 80), "halo_is_bias": ((1, 24, 48), 143, 40),
                  "seam_is_border": (_BIG, 5, 135), "fc1_high_channel_dropped": (_BIG, 5, 135), "fc2_moved": (_BIG, 0, 40),
                  "corner_clamped": ((2, 9, 17), 143, 163)},
    ("v3", 180): {"tap_moved": (_BIG, 179, 80), "swap_a_gate": (_BIG, 179, 80), "dw_bias_dropped": (_BIG, 5, 80), "halo_is_bias": (_BIG, 179, 20),
                  "seam_is_border": (_BIG, 5, 135), "fc1_high_channel_dropped": (_BIG, 179, 155), "fc2_moved": (_BIG, 179, 80),
                  "corner_clamped": ((2, 9, 17), 5, 139)},
}


def worst_ratio(got_upd, ref_upd, tau: float):
    """(max over elements of |got - ref| / (tau (|ref| + 1)), the element's index): <= 1 passes."""
    r = (got_upd - ref_upd).abs() / (tau * (ref_upd.abs() + 1.0))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def assert_update(got_upd, ref_upd, tau: float, what: str, geom, show: int = 6):
    """Every element of the update within tau (|ref| + 1); the failing elements by (b, y, x, c).  Returns the worst err / bar."""
    B, H, W = geom
    got_upd, ref_upd = got_upd.reshape(B, H, W, -1), ref_upd.reshape(B, H, W, -1)
    assert torch.isfinite(got_upd).all(), what + ": non-finite output"
    ratio, _ = worst_ratio(got_upd, ref_upd, tau)
    if ratio > 1.0:
        bad = ((got_upd - ref_upd).abs() > tau * (ref_upd.abs() + 1.0)).nonzero()
        lines = [f"(b={i[0]}, y={i[1]}, x={i[2]}, c={i[3]}): got {float(got_upd[tuple(i)]):.5g} want {float(ref_upd[tuple(i)]):.5g}" for i in bad[:show].tolist()]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got_upd.numel()} elements of the update are beyond tau = {tau} (worst {ratio:.2f} x the bar): "
                             + "; ".join(lines))
    return ratio


# ------------------------------------------------------------------------------------------------
# hat_ocab_qkv (linear: on the lattice) and hat_ocab_mlp (lattice fc1, GELU, selector fc2)
# ------------------------------------------------------------------------------------------------
QKV_NPIX = [15, 16, 136]
QSCALE = 0.5


@functools.lru_cache(maxsize=None)
def qkv_case(npix: int) -> L.Case:
    """[q * qscale | k | v] = x . [Wq qscale ; Wkv]^T + [bq qscale ; bkv] over npix pixels of 144 channels, all on the lattice."""
    key = "ocab_qkv"
    c = L.Case(npix=npix)
    c.x = L.acts(f"{key}.x{npix}", (1, 1, npix, 144))
    c.wq, c.wkv = L.weights(key + ".wq", (144, 144)), L.weights(key + ".wkv", (288, 144))
    c.bq, c.bkv = L.draw(key + ".bq", (144,), 8), L.draw(key + ".bkv", (288,), 8)
    Wm, b = torch.cat([c.wq * QSCALE, c.wkv]), torch.cat([c.bq * QSCALE, c.bkv])
    c.ref = c.x @ Wm.t() + b
    L.assert_exact_domain(f"{key} {npix}", stored=[("x", c.x, torch.bfloat16), ("W", Wm, torch.bfloat16), ("b", b, torch.float32)],
                          absum=c.x.abs() @ Wm.abs().t() + b.abs(), unit=0.5, addends=[b, c.ref])
    return c


def qkv_fragments_hit(c: L.Case):
    """(27 n-tiles, 5 k-steps) -> whether the stacked weight has a non-zero in that fragment (k-step 4 is the 16-deep half step)."""
    Wm = torch.cat([c.wq, c.wkv])
    return torch.stack([torch.stack([(Wm[16 * nt:16 * nt + 16, 32 * ks:min(32 * ks + 32, 144)] != 0).any() for ks in range(5)]) for nt in range(27)])


MLP_GEOM = (2, 3, 23)             # 138 pixels: 8 full 16-pixel tiles and a ragged one, a sample boundary inside a tile
MLP_SHIFTS = [17 * i for i in range(9)]


def mlp_fc2(shift: int):
    """fc2 (144, 288) with ONE power of two per column: column k at channel (k + shift) mod 144."""
    k = torch.arange(288)
    W2 = torch.zeros(144, 288, dtype=torch.float64)
    W2[(k + shift) % 144, k] = 2.0 ** ((k % 3) - 1).double() * (1 - 2 * ((k // 3) % 2)).double()
    return W2


def mlp_fragments_hit(shifts):
    """(9 n-tiles, 9 k-steps) -> whether some probe of `shifts` has a non-zero fc2 weight in that fragment (k-step kk = hidden units
    32 kk .. 32 kk + 31)."""
    hit = torch.zeros(9, 9, dtype=torch.bool)
    for s in shifts:
        nz = mlp_fc2(s) != 0
        hit |= nz.reshape(9, 16, 9, 32).any(3).any(1)
    return hit


@functools.lru_cache(maxsize=None)
def mlp_case(geom=MLP_GEOM) -> L.Case:
    """x, fc1 (on the lattice, |S| <= 4), b1, r1 (dyadic, exact in FP16), b2; S = fc1(x) + b1 exactly."""
    B, H, W = geom
    key = f"ocab_mlp{geom}"
    c = L.Case(geom=geom)
    c.x = L.acts(key + ".x", (B, H, W, 144))
    w1, b1 = L.weights("ocab_mlp.w1", (288, 144)), L.draw("ocab_mlp.b1", (288,), 8)
    s_int = c.x @ w1.t() + b1
    c.s = L.act_step(s_int)
    c.w1, c.b1, c.S = w1 * 2.0 ** -c.s, b1 * 2.0 ** -c.s, s_int * 2.0 ** -c.s
    c.r1 = L.draw(key + ".r1", (B, H, W, 144), 64, 2)
    c.b2 = L.draw("ocab_mlp.b2", (144,), 8, 2)
    assert float(c.S.abs().max()) <= 4.0
    L.assert_exact_domain(key, stored=[("x", c.x, torch.bfloat16), ("w1", c.w1, torch.bfloat16), ("b1", c.b1, torch.float32),
                                       ("r1", c.r1, torch.float16), ("b2", c.b2, torch.float32)],
                          absum=c.x.abs() @ c.w1.abs().t() + c.b1.abs(), unit=2.0 ** -c.s, addends=[c.b1, c.S])
    return c


def bf16_ulp(h: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 numbers at h (fp64 tensor of bf16 values)."""
    e = torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -126)))
    return torch.where(h == 0, 0.0, 2.0 ** (e - 7))


def mlp_expect(c: L.Case, W2: torch.Tensor):
    """(lo, hi) in fp64: the band r1 + b2 + sum_k w_k h_k with every hidden value h_k within ONE bf16 ulp of GELU(S_k) (the lattice
    suite's rule behind an activation: GELU(S) through fp32 to bf16), each scaled by its |w_k|, plus the fp32 round-off of the few
    additions that form the result (2^-21 of the terms' magnitudes)."""
    h = r_bf16(L.act64(c.S, 1))
    mid = c.r1 + c.b2 + h @ W2.t()
    mag = c.r1.abs() + c.b2.abs() + h.abs() @ W2.abs().t()
    tol = bf16_ulp(h) @ W2.abs().t() + mag * 2.0 ** -21
    return mid - tol, mid + tol


def assert_band(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, what: str, show: int = 6):
    """lo <= got <= hi after lo and hi are rounded to got's type (rounding is monotonic: a value of the band rounds into it)."""
    got = got.detach().cpu()
    assert torch.isfinite(got.float()).all(), what + ": non-finite output"
    lo_t, hi_t = lo.to(torch.float32).to(got.dtype).double(), hi.to(torch.float32).to(got.dtype).double()
    bad = (got.double() < lo_t) | (got.double() > hi_t)
    if bad.any():
        idx = bad.nonzero()
        lines = [f"{tuple(i)}: got {float(got[tuple(i)])!r} band [{float(lo_t[tuple(i)])!r}, {float(hi_t[tuple(i)])!r}]" for i in idx[:show].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside the one-ulp band; first: " + "; ".join(lines))
