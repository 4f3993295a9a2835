"""Structural probes of the HAB tail kernels and the OCAB MLP / QKV (tests/probes.py; DESIGN "Structural probes"), THROUGH THE C ABI.

Stage 0 of hat_hab_tail / hat_hab_tail3 (aggregation, folded CAB or scaled c2 map, residuals) is linear: on lattice operands tB is
an exact fp32 number, so with fc2 = 0 the kernels must return tB + b2 BIT FOR BIT, and with selector FFN weights the update
t_out - tB is isolated exactly and judged element by element against the oracle's fp64 gated FFN:  |got - ref| <= tau (|ref| + 1),
tau from probes.TAU (four times the emulated storage roundings, never from a kernel's output).  hat_ocab_qkv is linear and sits on
the lattice; hat_ocab_mlp has a lattice fc1 and a selector fc2 and is held to one bf16 ulp of GELU(S) per hidden value.
test_probes_cpu.py checks the domains, the bars, the coverage of the shift sets and that the mutants fail these judgements."""
import pytest
import torch
import torch.nn.functional as F

import lattice as L
import probes as P
from helpers import check, fill_rows

pytestmark = pytest.mark.gpu

KERNELS = {"ffn2": ("v2", 144), "tail_v2": ("v2", 144), "tail3": ("v3", 144), "tail3l": ("v3", 180)}
_GEOM_ID = lambda g: "x".join(map(str, g))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def _rows(x_bhwc, ld, tdt, dev):
    return fill_rows(x_bhwc.to(torch.float32), ld, tdt, dev, L.POISON)


_STAGE0 = {}


def _stage0(C, geom):
    """The lattice case of (C, geom) and its device operands: input pad channels hold the poison."""
    if (C, geom) in _STAGE0:
        return _STAGE0[(C, geom)]
    dev, ops = _dev(), _ops()
    from super_resolution_amd import packing
    c = P.stage0_case(C, geom)
    B, H, W = geom
    bf = torch.bfloat16
    d = dict(pw=ops.pack_linear_weight(c.wa.float(), None, ops.HAT_BF16, dev), y16=_rows(c.y16, 16, bf, dev),
             t=c.t.float().reshape(B, H * W, C).to(dev).contiguous(), tB=c.ref.reshape(B, H * W, C))
    pw = d["pw"]
    if C == 144:
        assert (pw.nt, pw.kpad) == (9, 160)
        d["ldn_in"] = C + 8
        # wf as hat_cab_fold writes it: [co][tap * 8 + ci] fragments, with the folded bias in k-slot 72 ("tap 9": bf16 head; its
        # remainder in slot 73 is zero for a dyadic bias).  hat_hab_tail3 takes the bias from there, hat_hab_tail from bias_b.
        full = torch.zeros(B, C, 12, 8)
        full[:, :, :9, :c.mid] = c.wf.float().reshape(B, C, c.mid, 9).permute(0, 1, 3, 2)
        full[:, :, 9, 0] = c.bias_b.float()
        d["wf"] = torch.stack([packing.frags(full[b].reshape(C, 96)).reshape(-1) for b in range(B)]).to(bf).to(dev).contiguous()
        assert d["wf"].shape == (B, pw.nt * 3 * 512)
        d["bias_b"] = torch.zeros(B, pw.npad, device=dev)
        d["bias_b"][:, :C] = c.bias_b.float().to(dev)
        d["c1"] = _rows(c.c1, 8, bf, dev)
    else:
        assert (pw.nt, pw.kpad) == (12, 192)
        d["ldn_in"] = 184
        d["c2"] = _rows(c.c2, 184, bf, dev)
        sc = torch.full((B * 192 + 64,), L.POISON, device=dev)          # rows of 192 floats, 1 KiB readable from every row's start
        sc[:B * 192].view(B, 192)[:, :C] = c.r2scale.float().to(dev)     # (floats 180..191 of a row belong to the dead lanes)
        d["scale"] = sc
        d["bias"] = torch.zeros(256, device=dev)
        d["bias"][:C] = c.bias.float().to(dev)
    d["n"] = _rows(c.n, d["ldn_in"], bf, dev)
    _STAGE0[(C, geom)] = (c, d)
    return c, d


def _pack(kernel, sd, dev):
    ops = _ops()
    f = lambda k: sd[k].float()
    args = (f("m.fc1.weight"), f("m.fc1.bias"), f("m.dw.weight"), f("m.dw.bias"), f("m.fc2.weight"), f("m.fc2.bias"))
    if kernel in ("ffn2", "tail_v2"):
        return ops.pack_ffn2(*args, dev)
    return ops.pack_ffn3(*args, f("n2.weight"), f("n2.bias"), dev)


def _launch(kernel, geom, sd, in_half=False, out_half=False):
    """One launch of `kernel` on the lattice stage-0 operands of `geom` with the FFN weights `sd`.  Returns (t_out (B, N, C) on the
    host, the next LayerNorm rows n_out (B, N, ldn) with their pad channels, n16 or None, the exact tB)."""
    dev, ops = _dev(), _ops()
    C = KERNELS[kernel][1]
    c, d = _stage0(C, geom)
    B, H, W = geom
    N = H * W
    bf = torch.bfloat16
    pf = _pack(kernel, sd, dev)
    dv = lambda k: sd[k].float().to(dev).contiguous()
    ldn = 184 if C == 180 else C + 8
    tiles = -(-H // 8) * -(-W // 16)
    n_out = torch.full((B, N, ldn), L.FILL, dtype=bf, device=dev)
    gap = torch.zeros(B, tiles, 16, device=dev)
    out = torch.full((B, N, C), L.FILL, dtype=torch.float16 if out_half else torch.float32, device=dev)
    kw = dict(B=B, H=H, W=W, dtype=ops.HAT_BF16, ln1=(dv("n1.weight"), dv("n1.bias")), n_out=n_out, ldn=ldn, gap_out=gap, gap_c=16)
    n16 = None
    if kernel == "ffn2":
        t_in = c.ref.float().reshape(B, N, C).to(dev).contiguous()      # tB itself: an fp32 number by the lattice's domain condition
        ops.ffn(pf, t_in, out, dv("n2.weight"), dv("n2.bias"), **kw)
    else:
        n16 = torch.full((B, N, 16), L.FILL, dtype=bf, device=dev)
        t_in = d["t"].half() if in_half else d["t"]
        assert ops.hab_tail_supported(pf, d["pw"], 6 if C == 144 else 60, ops.HAT_BF16)
        if C == 144:
            ops.hab_tail(pf, d["pw"], t_in, out, dv("n2.weight"), dv("n2.bias"), n=d["n"], ldn_in=d["ldn_in"], y16=d["y16"], c1=d["c1"], wf=d["wf"],
                         bias_b=d["bias_b"], n16_out=n16, **kw)
        else:
            ops.hab_tail(pf, d["pw"], t_in, out, dv("n2.weight"), dv("n2.bias"), n=d["n"], ldn_in=d["ldn_in"], y16=d["y16"], bias_b=d["bias"],
                         r2=d["c2"], ldr2=184, r2scale=d["scale"], r2scale_bstride=192, n16_out=n16, **kw)
    torch.cuda.synchronize()
    return out.cpu(), n_out.cpu(), (None if n16 is None else n16.cpu()), d["tB"]


def _check_next_ln(kernel, t_out, n_out, n16, sd, what):
    """The epilogue's LayerNorm rows against fp64 LayerNorm of the kernel's OWN t_out; their pad channels keep the fill; the compact
    copy is the first 16 channels bit for bit."""
    C = KERNELS[kernel][1]
    want = F.layer_norm(t_out.double(), (C,), sd["n1.weight"], sd["n1.bias"], 1e-5)
    check(n_out[:, :, :C].float(), want, "bf16", what + " next LayerNorm")
    assert torch.all(n_out[:, :, C:] == L.FILL), what + ": pad channels of n_out keep the fill"
    if n16 is not None:
        assert torch.equal(n16, n_out[:, :, :16].contiguous()), what + ": compact 16-channel copy"


# ------------------------------------------------------------------------------------------------
# stage 0, bit-exact (fc2 = 0)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", P.SHAPES, ids=_GEOM_ID)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_stage0_is_exact(kernel, geom):
    """fc2 = 0: t_out == tB + b2 bit for bit — hat_ffn2 alone returns t_in + b2, hat_hab_tail / hat_hab_tail3 their fused stage 0
    (aggregation, y16 channel split, folded-CAB im2col with per-sample wf and bias_b at 144; r2 * r2scale and ldn_in = 184 at 180)."""
    C = KERNELS[kernel][1]
    sd = P.selector_ffn(C, 3, zero_fc2=True)
    B, H, W = geom
    t_out, n_out, n16, tB = _launch(kernel, geom, sd)
    want = L.expect(tB + sd["m.fc2.bias"], torch.float32)
    L.assert_bits(t_out.reshape(B, H, W, C), want.reshape(B, H, W, C), f"{kernel} {geom}: t_out = tB + b2")
    _check_next_ln(kernel, t_out, n_out, n16, sd, f"{kernel} {geom}")


@pytest.mark.parametrize("geom", P.SHAPES, ids=_GEOM_ID)
def test_stage0_fp16_streams_are_exact(geom):
    """hat_hab_tail3 at 144 with the residual stream as FP16 rows: FP16 in is exact (t survives FP16), FP16 out is ONE
    round-to-nearest-even of tB + b2; the LayerNorm rows do not depend on the stream's type."""
    sd = P.selector_ffn(144, 3, zero_fc2=True)
    B, H, W = geom
    P.stage0_fp16_ok(P.stage0_case(144, geom))
    base = _launch("tail3", geom, sd)
    for in_half, out_half in [(True, False), (False, True), (True, True)]:
        t_out, n_out, n16, tB = _launch("tail3", geom, sd, in_half, out_half)
        want = L.expect(tB + sd["m.fc2.bias"], torch.float16 if out_half else torch.float32)
        L.assert_bits(t_out.reshape(B, H, W, 144), want.reshape(B, H, W, 144), f"tail3 {geom} FP16 in={in_half} out={out_half}")
        assert torch.equal(n_out, base[1]) and torch.equal(n16, base[2]), (geom, in_half, out_half)


# ------------------------------------------------------------------------------------------------
# the gated path, per element
# ------------------------------------------------------------------------------------------------
def _probe(kernel, geom, shifts):
    gen, C = KERNELS[kernel]
    B, H, W = geom
    tau, worst = P.TAU[(gen, C)], 0.0
    for s in shifts:
        sd = P.selector_ffn(C, s)
        t_out, n_out, n16, tB = _launch(kernel, geom, sd)
        ref = P.reference_update(tB, sd, (H, W))
        worst = max(worst, P.assert_update(t_out.double() - tB, ref, tau, f"{kernel} {geom} shift {s}", geom))
        _check_next_ln(kernel, t_out, n_out, n16, sd, f"{kernel} {geom} shift {s}")
    print(f"PROBE {kernel} {_GEOM_ID(geom)} shifts={len(shifts)} tau={tau} worst err/bar={worst:.3f}")


@pytest.mark.parametrize("geom", P.SHAPES, ids=_GEOM_ID)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gated_update_per_element(kernel, geom):
    """Selector weights at shifts {0, 5, C - 1}: every element of t_out - tB within tau (|ref| + 1) of the oracle's fp64 gated FFN."""
    _probe(kernel, geom, P.few_shifts(KERNELS[kernel][1]))


@pytest.mark.parametrize("kernel", ["tail3", "tail3l"])
def test_gated_update_covering_shifts(kernel):
    """The covering shift set on 2 x 2 tiles: every fc1 (unit, channel), fc2 (channel, unit) and (unit, tap) pair is non-zero in one
    of these launches (test_probes_cpu.py), among them the half-empty last k-step and, at 180, the neighbours of the dead units."""
    _probe(kernel, P.FULL_SHAPE, P.covering_shifts(KERNELS[kernel][1]))


# ------------------------------------------------------------------------------------------------
# hat_ocab_qkv on the lattice
# ------------------------------------------------------------------------------------------------
def _qkv(npix):
    dev, ops = _dev(), _ops()
    c = P.qkv_case(npix)
    bf = torch.bfloat16
    pm = ops.pack_ocab_qkv(c.wq.float(), c.bq.float(), c.wkv.float(), c.bkv.float(), P.QSCALE, dev)
    ldx, ldo = 152, 440
    x = _rows(c.x, ldx, bf, dev)
    out = torch.full((1, npix, ldo), L.FILL, dtype=bf, device=dev)
    ops.ocab_qkv(pm, x, out, B=1, H=1, W=npix, ldx=ldx, ldo=ldo, dtype=ops.HAT_BF16)
    torch.cuda.synchronize()
    L.assert_bits(out[:, :, :432].reshape(1, 1, npix, 432), L.expect(c.ref, bf), f"hat_ocab_qkv {npix} pixels")
    assert torch.all(out[:, :, 432:] == L.FILL), "pad channels of the output keep the fill"


@pytest.mark.parametrize("npix", P.QKV_NPIX)
def test_ocab_qkv_is_exact(npix):
    """[q * qscale | k | v] == the fp64 sum rounded once to bf16; padded ldx / ldo with poison and fill."""
    _qkv(npix)


def test_ocab_qkv_is_exact_over_two_trips():
    """More tiles than one trip of the persistent grid takes (test_gpu_multitrip.QKV_TRIP_TILES = 256 x 8): some waves take two."""
    from helpers import need_trips
    npix = 256 * 8 * 16 + 16 * 300 + 7
    need_trips(-(-npix // 16), 256 * 8, 2, "hat_ocab_qkv")
    _qkv(npix)


# ------------------------------------------------------------------------------------------------
# hat_ocab_mlp: lattice fc1, GELU, selector fc2
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32_r1_f32", "f32_inplace", "rows_r1_f32", "rows_r1_fp16"])
def test_ocab_mlp_selector(mode):
    """out = r1 + b2 + sum_k w_k bf16(GELU(S_k)) with S exact and ONE power-of-two fc2 weight per hidden unit, shifted so that every
    (n-tile, k-step) fragment of fc2 routes a value (the four register-resident ones included): within one bf16 ulp of GELU(S) per
    hidden value, scaled by its weight."""
    dev, ops = _dev(), _ops()
    c = P.mlp_case()
    B, H, W = c.geom
    N, C, bf = H * W, 144, torch.bfloat16
    x = _rows(c.x, C + 8, bf, dev)
    out_f32 = mode.startswith("f32")
    for s in P.MLP_SHIFTS:
        W2 = P.mlp_fc2(s)
        pm = ops.pack_ocab_mlp(c.w1.float(), c.b1.float(), W2.float(), c.b2.float(), dev)
        r1 = _rows(c.r1, C + 8, torch.float16 if mode == "rows_r1_fp16" else torch.float32, dev)
        out = r1 if mode == "f32_inplace" else torch.full((B, N, C + 8), L.FILL, dtype=torch.float32 if out_f32 else bf, device=dev)
        ops.ocab_mlp(pm, x, r1, out, B=B, H=H, W=W, ldx=C + 8, ldr1=C + 8, ldo=C + 8, out_f32=out_f32, dtype=ops.HAT_BF16)
        torch.cuda.synchronize()
        lo, hi = P.mlp_expect(c, W2)
        P.assert_band(out[:, :, :C].reshape(B, H, W, C), lo, hi, f"hat_ocab_mlp {mode} shift {s}")
        assert torch.all(out[:, :, C:] == (L.POISON if mode == "f32_inplace" else L.FILL)), f"{mode}: pad channels of the output are untouched"
