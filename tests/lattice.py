"""Exact-lattice parity (DESIGN "Exact-lattice parity tests"): operands on a small dyadic lattice make a linear kernel's result the
ONE exactly representable fp32 number, whatever its tiling, k-split or MFMA shape, so the fp64 reference (rounded once to the
output type) is the only answer the kernel may give.  Host only: seeded lattice draws, the domain condition, the once-rounded
expectation, the bit / one-ulp comparisons, fp64 references, and the case tables that test_gpu_lattice.py launches and
test_lattice_cpu.py checks the domain of.  Nothing here loads the library or touches a GPU."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from super_resolution_amd import synth
from super_resolution_amd.packing import choose_nt, choose_nt_linear

SEED = 29
POISON = 7.0                      # pad channels of the inputs: finite (a pad channel under a zero weight may be multiplied), never read into a sum
FILL = 3.0                        # outputs before the launch
LIMIT = float(2 ** 24)            # lattice steps a sum may span and stay exact in fp32
MEAN = (0.5, 0.25, 0.375)         # dyadic `mean`
STORE = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}


# ------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------
def draw(key: str, shape, a: int, s: int = 0, density: float = 1.0) -> torch.Tensor:
    """fp64 tensor of integers in [-a, a] times 2^-s; an element is nonzero with probability `density` (times 2a / (2a + 1)).
    A pure function of (SEED, key, element index)."""
    n = int(np.prod(shape)) if len(shape) else 1
    v = np.floor(synth._uniform01(SEED, key, n, 3) * (2 * a + 1)) - a
    if density < 1.0:
        v = v * (synth._uniform01(SEED, key, n, 4) < density)
    return torch.from_numpy((v * 2.0 ** -s).reshape(tuple(shape)))


def acts(key, shape, s: int = 0):
    """Activations: a = 4."""
    return draw(key, shape, 4, s)


def weights(key, shape, s: int = 0, density: float = 0.5):
    """Weights: a = 2 at density 0.25 - 0.5."""
    return draw(key, shape, 2, s, density)


# ------------------------------------------------------------------------------------------------
# the domain condition, the expectation, the comparisons
# ------------------------------------------------------------------------------------------------
def assert_exact_domain(what: str, *, stored, absum, unit: float, addends=()):
    """The conditions under which `what` is exact, checked on the host for the case at hand (a violation is a bug of the TEST and
    raises): every (name, tensor, dtype) of `stored` survives the round trip through its storage type unchanged; every tensor of
    `addends` (biases, residuals, scaled residuals, the reference itself) is a whole number of `unit`s, the step of the result's
    lattice; and absum = sum |x| |w| + |bias| + |residuals| (a tensor or a bound that holds for every output) stays below 2^24
    units, so that every partial sum in any order is an exactly representable fp32 number."""
    for name, t, dt in stored:
        t = torch.as_tensor(t, dtype=torch.float64)
        back = t.to(torch.float32).to(dt).to(torch.float64)
        if not torch.equal(back, t):
            raise AssertionError(f"{what}: operand {name} does not survive {dt}: {int((back != t).sum())} of {t.numel()} elements change")
    for i, t in enumerate(addends):
        r = torch.as_tensor(t, dtype=torch.float64) / unit
        if not torch.equal(r, r.round()):
            raise AssertionError(f"{what}: addend {i} is off the result lattice of step {unit}")
    top = float(torch.as_tensor(absum, dtype=torch.float64).max()) / unit
    if not top < LIMIT:
        raise AssertionError(f"{what}: sum of absolute terms spans {top:.4g} steps of {unit}, not below 2^24")


def expect(ref64: torch.Tensor, tdt) -> torch.Tensor:
    """The fp64 reference rounded ONCE, to nearest even, to the output's type (the reference must be an fp32 number already: the
    domain condition; the conversion fp32 -> bf16 / fp16 is then the single rounding the kernel's store performs)."""
    f = ref64.to(torch.float32)
    if not torch.equal(f.to(torch.float64), ref64):
        raise AssertionError("the reference is not exactly representable in fp32: the case is outside the exact domain")
    return f.to(tdt)


def _where(idx, shape):
    names = "byxc" if len(shape) == 4 else "".join(f"d{i}" for i in range(len(shape)))
    return "(" + ", ".join(f"{n}={int(v)}" for n, v in zip(names, idx)) + ")"


def assert_bits(got: torch.Tensor, want: torch.Tensor, what: str, show: int = 8):
    """got == want on the raw values (same dtype, same shape, no NaN).  On failure: how many elements differ and the first few
    indices — (b, y, x, c) for a 4-D tensor — with both values, so that a seam or a border pattern is visible."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    lines = [f"{_where(i, got.shape)}: got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx[:show]]
    span = ", ".join(f"{int(idx[:, d].min())}..{int(idx[:, d].max())}" for d in range(idx.shape[1]))
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ (index ranges {span}); first: " + "; ".join(lines))


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """The values' bit patterns as integers that count representable numbers in order (+-0 coincide)."""
    if t.dtype == torch.float32:
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    i = t.contiguous().view(torch.int16).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def assert_ulp(got: torch.Tensor, want: torch.Tensor, what: str, ulps: int = 1, show: int = 8):
    """Every element of got within `ulps` representable numbers of want (same dtype)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got.float()).all(), what + ": non-finite output"
    dist = (_ordered(got) - _ordered(want)).abs()
    bad = dist > ulps
    if bad.any():
        idx = bad.nonzero()
        lines = [f"{_where(i, got.shape)}: got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx[:show]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements are more than {ulps} ulp off (worst {int(dist.max())}); first: "
                             + "; ".join(lines))


# ------------------------------------------------------------------------------------------------
# fp64 references (channel-last maps)
# ------------------------------------------------------------------------------------------------
def conv64(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """'same' convolution, zero padding, stride 1, in fp64: x (B,H,W,Cin); w (Cout,Cin,k,k) or per-sample (B,Cout,Cin,k,k);
    -> (B,H,W,Cout)."""
    x = x.to(torch.float64).permute(0, 3, 1, 2)
    w = w.to(torch.float64)
    b = None if bias is None else bias.to(torch.float64)
    if w.dim() == 5:
        y = torch.cat([F.conv2d(x[i:i + 1], w[i], b, padding=w.shape[-1] // 2) for i in range(x.shape[0])], 0)
    else:
        y = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_abs(x, w, bias=None):
    """sum |x| |w| + |bias| per output: the left side of the domain bound."""
    return conv64(x.abs(), w.abs(), None if bias is None else bias.abs())


def act64(v: torch.Tensor, act: int) -> torch.Tensor:
    """HAT_ACT_NONE / GELU (erf) / LRELU (slope 0.01) in fp64."""
    if act == 1:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == 2:
        return torch.where(v >= 0, v, 0.01 * v)
    assert act == 0
    return v


def pixel_shuffle_last(y: torch.Tensor, r: int) -> torch.Tensor:
    """nn.PixelShuffle(r) on a channel-last map: (B,H,W,C r^2) -> (B,rH,rW,C)."""
    return F.pixel_shuffle(y.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1).contiguous()


def upfold_ref64(x, wu, bu, wl, bl, out_scale, mean):
    """Conv2d(64, 256, 3) -> PixelShuffle(2) -> Conv2d(64, 3, 3), then v * out_scale + mean, in fp64: x (B,H,W,64) -> (B,3,2H,2W).
    The three operations themselves, NOT packing.upfold_apply: the packer's border variants are under test too."""
    y = conv64(pixel_shuffle_last(conv64(x, wu, bu), 2), wl, bl)
    return (y * out_scale + torch.tensor(mean, dtype=torch.float64)).permute(0, 3, 1, 2).contiguous()


def ring_mask(h: int, w: int) -> torch.Tensor:
    """The outermost pixels of an (h, w) map."""
    m = torch.ones(h, w, dtype=torch.bool)
    m[1:-1, 1:-1] = False
    return m


def act_step(s_int: torch.Tensor) -> int:
    """The weight step 2^-s at which the sums S = s_int 2^-s obey |S| <= 4: the range over which an activation's kernel is
    compared (erf-GELU's error bound of 1.5e-7 stays below half a bf16 ulp of GELU(S) there)."""
    top = float(s_int.abs().max())
    return max(0, math.ceil(math.log2(max(top, 1.0) / 4.0)))


# ------------------------------------------------------------------------------------------------
# case tables.  Geometry (B, H, W): B = 2 with ragged last tiles in both directions, a frame smaller than one tile, one exact tile.
# ------------------------------------------------------------------------------------------------
GEOMS = [(2, 19, 21), (1, 3, 5), (1, 16, 16)]
DTYPES = ["bf16", "f32"]

# hat_conv, plain (HAT_O_NHWC_T, n_store = round4(Cout)): (k, Cin, Cout)
CONV_PLAIN = [(3, 144, 144), (3, 180, 180), (3, 64, 64), (3, 64, 12), (3, 64, 27), (3, 64, 48), (13, 16, 16), (5, 8, 8)]

# hat_conv, one epilogue / input / output form each.  Fields: name, (B,H,W), k, Cin, Cout, dtypes, and the options conv_case reads.
ConvForm = namedtuple("ConvForm", "name geom k cin cout dtypes opt")
CONV_FORMS = [
    ConvForm("r1_f32", (2, 19, 21), 3, 144, 144, DTYPES, dict(out="f32", r1="f32")),
    ConvForm("r1_inplace", (2, 19, 21), 3, 144, 144, DTYPES, dict(out="f32", r1="inplace")),
    ConvForm("r1_r2_x0_colsum_k1", (2, 19, 21), 1, 144, 144, DTYPES, dict(out="f32", r1="f32", r2=True, c_split=16, colsum=True)),
    ConvForm("x0_split", (2, 19, 21), 3, 144, 144, DTYPES, dict(c_split=16)),
    ConvForm("nchw_first", (2, 19, 21), 3, 3, 144, DTYPES, dict(x="nchw_mean", out="f32")),
    ConvForm("nchw_first_tiny", (1, 3, 5), 3, 3, 144, DTYPES, dict(x="nchw_mean", out="f32")),
    ConvForm("f32_source", (2, 19, 21), 3, 144, 144, DTYPES, dict(x="f32", out="f32", r1="inplace")),
    ConvForm("pixshuf2_resident", (1, 16, 16), 3, 64, 256, DTYPES, dict(out="ps", ps_r=2)),            # bf16: hat_conv64r
    ConvForm("pixshuf2_generic", (1, 16, 16), 3, 64, 256, DTYPES, dict(out="ps", ps_r=2, c_split=8)),  # x0: outside hat_conv64r
    ConvForm("pixshuf2_ragged", (2, 19, 21), 3, 64, 256, DTYPES, dict(out="ps", ps_r=2)),
    ConvForm("pixshuf3", (2, 19, 21), 3, 64, 576, DTYPES, dict(out="ps", ps_r=3)),
    ConvForm("pixshuf3_tiny", (1, 3, 5), 3, 64, 576, DTYPES, dict(out="ps", ps_r=3)),
    ConvForm("nhwc_f32", (2, 19, 21), 3, 64, 64, DTYPES, dict(out="f32")),
    ConvForm("nchw_last", (2, 19, 21), 3, 64, 3, DTYPES, dict(out="nchw")),
    ConvForm("colsum", (2, 19, 21), 3, 144, 144, DTYPES, dict(colsum=True)),
    ConvForm("colsum_6", (2, 19, 21), 3, 144, 6, DTYPES, dict(colsum=True)),
    ConvForm("fp16_r1", (2, 19, 21), 3, 144, 144, ["bf16"], dict(out="f32", r1="f16")),
    ConvForm("fp16_out", (2, 19, 21), 3, 144, 144, ["bf16"], dict(out="f16", r1="f32")),
    ConvForm("fp16_both_inplace", (2, 19, 21), 3, 144, 144, ["bf16"], dict(out="f16", r1="inplace")),
    ConvForm("fp16_both_tiny", (1, 3, 5), 3, 144, 144, ["bf16"], dict(out="f16", r1="f16")),
    ConvForm("layernorm_n16", (2, 19, 21), 3, 144, 144, DTYPES, dict(out="f32", r1="inplace", ln=True)),
    ConvForm("layernorm_fp16", (2, 19, 21), 3, 144, 144, ["bf16"], dict(out="f16", r1="inplace", ln=True)),
    # pointwise activations: GELU on the bf16 instantiation only (conv_case's docstring), LeakyReLU(0.01) on both
    ConvForm("gelu", (2, 19, 21), 3, 144, 144, ["bf16"], dict(act=1)),
    ConvForm("gelu_6", (2, 19, 21), 3, 144, 6, ["bf16"], dict(act=1)),
    ConvForm("lrelu", (2, 19, 21), 3, 144, 64, DTYPES, dict(act=2)),
    ConvForm("lrelu_resident", (2, 19, 21), 3, 64, 64, DTYPES, dict(act=2)),                            # bf16: hat_conv64r's epilogue
]

# hat_linear: (name, Cin, Cout); between them every (nt, ceil(Cin / 32)) of ops._PW_SHAPES in bf16 (test_lattice_cpu.py checks that)
LIN_SHAPES = [("aggr144", 144, 144), ("kv288", 144, 288), ("mlp2_288", 288, 144), ("lin180", 180, 180), ("mlp360", 360, 180),
              ("kv360", 180, 360), ("tiny24", 24, 48), ("tiny48", 48, 24), ("esc_out", 64, 64)]
LIN_GEOMS = [(1, 3, 5), (2, 19, 27)]
LIN_FORMS = {"plain": dict(), "residuals": dict(out="f32", r1="inplace", r2=True, c_split=8), "gelu": dict(act=1), "lrelu": dict(act=2)}
LIN_FP16 = {"fp16_r1": dict(out="f32", r1="f16"), "fp16_out": dict(out="f16", r1="f32"), "fp16_both_inplace": dict(out="f16", r1="inplace")}

# hat_conv3x3_small: (name, Cin, Cout), the four (nt, Cin_p) of ops._T3_SHAPES
T3_SHAPES = [("cab0", 144, 6), ("cab2", 6, 144), ("t_cab0", 24, 8), ("t_cab2", 8, 24)]
T3_GEOM = (2, 19, 21)

AGGR_GEOMS = [(2, 24, 40), (1, 19, 27)]
ESC13_GEOMS = [(1, 8, 8), (2, 45, 70), (1, 33, 129)]
SWEEP_GEOMS = [(2, 19, 32), (1, 9, 112), (1, 12, 272)]
SQUEEZE_CM = [(136, 8), (144, 6), (160, 3)]
UPFOLD_SHAPES = [(1, 16), (2, 16), (3, 16), (11, 32), (3, 4144)]      # (H, W) at B = 2


def resident_kernel_takes(dtype: str, k: int, cin: int, cout: int, opt) -> bool:
    """hat_conv hands a launch to the resident-weight kernel (hat_conv64r) when: bf16, 3 x 3 over 64 channels from one T source, a
    multiple of 64 outputs all stored, no residual / column sums / LayerNorm, no activation or LeakyReLU(0.01), T rows or pixel
    shuffle out.  Restated here so that the tables can show a case on either side of it.  The C predicate is hat_conv64r_can_launch
    (csrc/hat_conv64r.hip), which is not part of the C ABI, so nothing ties this copy to it: if it changes, change this with it, or
    a "resident" case moves to the generic kernel unnoticed (it stays bit-exact there; only the coverage claim is lost).  Not
    mirrored because every hat_conv case of these tables meets them: n_store == n_slices * nt * 16 (a multiple of 64 outputs, all
    stored), Kpad >= 576 (pack_conv_weight's padding of 9 * 64), w_bstride == 0, no gap_out, ldx % 8 == 0 (ldx = 72)."""
    o = dict(x="T", out="T", r1=None, r2=False, c_split=0, colsum=False, ln=False, act=0)
    o.update(opt or {})
    return (dtype == "bf16" and k == 3 and cin == 64 and cout % 64 == 0 and o["x"] == "T" and not o["c_split"] and not o["r1"] and not o["r2"]
            and not o["colsum"] and not o["ln"] and o["act"] in (0, 2) and o["out"] in ("T", "ps"))


def conv64r_trip_tiles(nsl: int, ntiles: int):
    """csrc/hat_conv3_tile.h conv3_groups, which hat_conv64r_launch has no query for: `int m = 32 / nsl; if (m < 1) m = 1;
    while (m > 1 && 8LL * (m - 1) >= ntiles) --m;`, launched as nwps = 8 * m workgroups per slice
    -> (nwps: 16 x 16 tiles over B that the workgroups of one 64-channel slice cover per trip, m).
    test_srvgg_cpu.py holds it against the queries of the kernels that share the rule (hat_vgg_conv_tiles, hat_rdb_conv_tiles)."""
    m = max(32 // nsl, 1)
    while m > 1 and 8 * (m - 1) >= ntiles:
        m -= 1
    return 8 * m, m


def lin_dtypes(cin: int, cout: int):
    """The instantiations hat_linear has for a shape (the fp32 image of the widest weights does not fit the LDS)."""
    from super_resolution_amd import ops
    return [d for d in DTYPES if ops.linear_supported(cout, cin, ops.DTYPE_CODE[d])]


def t3_dtypes(cin: int, cout: int):
    from super_resolution_amd import ops
    return [d for d in DTYPES if ops.conv3x3_small_supported(cout, cin, ops.DTYPE_CODE[d])]


def pw_pair(cin: int, cout: int, dtype_code: int):
    """(nt, ceil(Cin / 32)): the hat_linear instantiation a shape runs on."""
    return choose_nt_linear(cout, cin, dtype_code)[0], -(-cin // 32)


def t3_pair(cin: int, cout: int):
    return choose_nt(cout)[0], (cin + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------
# operand builders: everything a launch needs, on the host in fp64, with the reference and the domain condition checked
# ------------------------------------------------------------------------------------------------
class Case:
    """Operands (fp64, exactly storable), the fp64 reference `ref` (before a pointwise activation: the exact sum S), and what the
    form adds (`colsum_ref`, ...)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def conv_case(key: str, geom, k: int, cin: int, cout: int, dtype: str, opt=None) -> Case:
    """One hat_conv / hat_linear / hat_conv3x3_small launch of the epilogue  v = act(acc + bias) + r1 + r2scale * r2.

    opt: x = "T" | "f32" (fp32 token rows) | "nchw_mean" ((x - mean) * in_scale from NCHW fp32);  out = "T" | "f32" | "f16" (FP16
    residual-stream rows) | "ps" (HAT_O_PIXSHUF_T, ps_r) | "nchw" (v * out_scale + mean);  r1 = None | "f32" | "inplace" | "f16";
    r2 (with a per-sample, per-channel dyadic r2scale);  c_split (channels [0, c_split) come from x0);  colsum;  ln (fused LayerNorm:
    the main output stays exact, ln_out is not on the lattice);  act.

    With act != 0 the weights and the bias take the step 2^-s at which |S| <= 4 everywhere, and `ref` is S: the expectation is
    act(S) in fp64 rounded once, met within one ulp.  GELU is compared on the bf16 instantiation only: its gelu_erf_fast documents
    |error| <= 1.5e-7, which can only flip a bf16 rounding, while the fp32 instantiation's erff-based GELU loses relative accuracy in
    1 + erf(x) for x < 0 by design (the operation torch performs in fp32 too) and is no one-ulp function of S; it stays on
    helpers.check's 2e-5 bar (test_gpu_ops.py)."""
    o = dict(x="T", out="T", r1=None, r2=False, c_split=0, colsum=False, ln=False, act=0, ps_r=0)
    o.update(opt or {})
    B, H, W = geom
    st = STORE[dtype]
    what = f"{key}[{dtype}]"
    c = Case(opt=o, geom=geom, k=k, cin=cin, cout=cout, dtype=dtype, in_scale=1.0, out_scale=1.0, mean=(0.0, 0.0, 0.0))
    x = acts(key + ".x", (B, H, W, cin))
    w = weights(key + ".w", (cout, cin, k, k), density=0.5 if cin * k * k <= 1296 else 0.25)
    bias = draw(key + ".b", (cout,), 8)
    c.x_in = x                                        # what the MFMA consumes
    if o["c_split"]:
        c.x0 = acts(key + ".x0", (B, H, W, o["c_split"]))
        c.x_in = torch.cat([c.x0, x[..., o["c_split"]:]], -1)
    if o["x"] == "nchw_mean":
        c.in_scale, c.mean = 0.5, MEAN
        c.x_src = (x / c.in_scale + torch.tensor(MEAN[:cin], dtype=torch.float64)).permute(0, 3, 1, 2).contiguous()     # fp32 planes
    s_int = conv64(c.x_in, w, bias)
    s = act_step(s_int) if o["act"] else 0
    w, bias = w * 2.0 ** -s, bias * 2.0 ** -s
    c.x, c.w, c.bias, c.s = x, w, bias, s
    ref = s_int * 2.0 ** -s
    absum = conv_abs(c.x_in, w, bias)
    unit = 2.0 ** -s
    stored = [("x", x, st), ("w", w, st), ("bias", bias, torch.float32)]     # (fp32 sources are converted to T before the MFMA)
    if o["c_split"]:
        stored.append(("x0", c.x0, st))
    if o["x"] == "nchw_mean":
        stored += [("x planes", c.x_src, torch.float32), ("(x - mean) * in_scale", x, st)]
    addends = [bias]
    if o["r1"]:
        c.r1 = draw(key + ".r1", (B, H, W, cout), 64, 2)
        stored.append(("r1", c.r1, torch.float16 if o["r1"] == "f16" or (o["r1"] == "inplace" and o["out"] == "f16") else torch.float32))
        ref, absum, unit = ref + c.r1, absum + c.r1.abs(), min(unit, 0.25)
        addends.append(c.r1)
    if o["r2"]:
        c.r2 = acts(key + ".r2", (B, H, W, cout), 1)
        c.r2scale = draw(key + ".sc", (B, cout), 6, 2)
        term = c.r2scale[:, None, None, :] * c.r2
        stored += [("r2", c.r2, st), ("r2scale", c.r2scale, torch.float32)]
        ref, absum, unit = ref + term, absum + term.abs(), min(unit, 0.125)
        addends.append(term)
    if o["out"] == "nchw":
        c.out_scale, c.mean = 0.5, MEAN
        m = torch.tensor(MEAN[:cout], dtype=torch.float64)
        ref, absum, unit = ref * 0.5 + m, absum * 0.5 + m.abs(), 0.125
        addends.append(m)
    assert_exact_domain(what, stored=stored, absum=absum, unit=unit, addends=addends + [ref])
    if o["act"]:
        assert float(ref.abs().max()) <= 4.0, (what, float(ref.abs().max()))
    c.ref, c.unit = ref, unit
    return c


def aggr_case(geom) -> Case:
    """hat_aggr_cab: out = r1 + W_aggr . [x0 | x] + wf_b . im2col3x3(c1) + bias_b, wf and bias_b per sample (what hat_cab_fold
    writes: here lattice numbers of their own, different for every b)."""
    B, H, W = geom
    C, mid, key = 144, 6, f"aggr{geom}"
    c = Case(geom=geom, C=C, mid=mid)
    c.x, c.x0 = acts(key + ".x", (B, H, W, C)), acts(key + ".x0", (B, H, W, 16))
    c.c1 = torch.zeros(B, H, W, 8, dtype=torch.float64)
    c.c1[..., :mid] = acts(key + ".c1", (B, H, W, mid), 1)
    c.wa = weights(key + ".wa", (C, C))
    c.wf = weights(key + ".wf", (B, C, mid, 3, 3), 2)
    c.bias_b = draw(key + ".bb", (B, C), 8, 2)
    c.r1 = draw(key + ".r1", (B, H, W, C), 64, 2)
    xin = torch.cat([c.x0, c.x[..., 16:]], -1)
    bb = c.bias_b[:, None, None, :]
    c.ref = c.r1 + conv64(xin, c.wa[:, :, None, None]) + conv64(c.c1[..., :mid], c.wf) + bb
    absum = c.r1.abs() + conv_abs(xin, c.wa[:, :, None, None]) + conv_abs(c.c1[..., :mid], c.wf) + bb.abs()
    bf = torch.bfloat16
    assert_exact_domain(key, stored=[("x", c.x, bf), ("x0", c.x0, bf), ("c1", c.c1, bf), ("wa", c.wa, bf), ("wf", c.wf, bf),
                                     ("bias_b", c.bias_b, torch.float32), ("r1", c.r1, torch.float32)],
                        absum=absum, unit=0.125, addends=[c.r1, c.bias_b, c.ref])
    return c


def esc13_case(geom) -> Case:
    """hat_esc_conv13: the 13 x 13 conv over the first 16 of 144 channels with per-sample weights (hat_esc_weights' layout)."""
    B, H, W = geom
    key = f"esc13{geom}"
    c = Case(geom=geom)
    c.x = acts(key + ".x", (B, H, W, 16))
    c.w = weights(key + ".w", (B, 16, 16, 13, 13), density=0.25)            # [b][co][ci][ty][tx], another draw for every b
    assert not torch.equal(c.w[0], c.w[-1]) or B == 1
    c.ref = conv64(c.x, c.w)
    assert_exact_domain(key, stored=[("x", c.x, torch.bfloat16), ("w", c.w, torch.bfloat16)], absum=conv_abs(c.x, c.w), unit=1.0, addends=[c.ref])
    return c


def sweep_case(geom, C: int, nout: int, gelu: bool) -> Case:
    """The row-sweep 3 x 3 kernel: hat_conv3x3_to_planes ((conv + bias) * out_scale + mean, exact) or hat_cab_squeeze (GELU(conv +
    bias): `ref` is the exact sum S, |S| <= 4)."""
    B, H, W = geom
    key = f"sweep{geom}.{C}.{nout}"
    c = Case(geom=geom, C=C, nout=nout)
    c.x = acts(key + ".x", (B, H, W, C))
    w = weights(key + ".w", (nout, C, 3, 3))
    bias = draw(key + ".b", (nout,), 8)
    s_int = conv64(c.x, w, bias)
    c.s = act_step(s_int) if gelu else 0
    c.w, c.bias = w * 2.0 ** -c.s, bias * 2.0 ** -c.s
    ref, absum, unit, add = s_int * 2.0 ** -c.s, conv_abs(c.x, c.w, c.bias), 2.0 ** -c.s, [c.bias]
    if gelu:
        assert float(ref.abs().max()) <= 4.0
    else:
        c.out_scale, c.mean = 0.5, MEAN
        m = torch.tensor(MEAN[:nout], dtype=torch.float64)
        ref, absum, unit = ref * 0.5 + m, absum * 0.5 + m.abs(), 0.125
        add.append(m)
    c.ref = ref
    assert_exact_domain(key, stored=[("x", c.x, torch.bfloat16), ("w", c.w, torch.bfloat16), ("bias", c.bias, torch.float32)], absum=absum,
                        unit=unit, addends=add + [ref])
    return c


def upfold_weights(key: str, density: float = 0.5):
    """(wu, bu, wl, bl) of the folded ending on the integer lattice: every one of the folded 5 x 5 variants is then a tensor of
    integers of at most 93 in magnitude (exact in bf16)."""
    return (weights(key + ".wu", (256, 64, 3, 3), density=density), draw(key + ".bu", (256,), 2),
            weights(key + ".wl", (3, 64, 3, 3), density=density), draw(key + ".bl", (3,), 8))


def upfold_case(shape, B: int = 2) -> Case:
    """hat_upfold_to_planes against the three operations in fp64.  The bound on the sum is taken over the weights alone (it
    holds for every pixel of any frame): the folded weights of an output are sums of products wl * wu."""
    from super_resolution_amd import packing
    H, W = shape
    key = f"upfold{shape}"
    c = Case(geom=(B, H, W), out_scale=0.5, mean=MEAN)
    c.x = acts(key + ".x", (B, H, W, 64))
    c.w = upfold_weights("upfold")
    wu, bu, wl, bl = c.w
    c.ref = upfold_ref64(c.x, wu, bu, wl, bl, c.out_scale, c.mean)
    G, Bd, b0 = packing.upfold_pieces(wu, bu, wl, bl)
    folded = [packing.upfold_variant(G, Bd, b0, rs, cs) for rs in range(4) for cs in range(3)]
    fw = torch.stack([f[0] for f in folded])
    per_mid = wu.abs().sum((1, 2, 3)) * 4.0 + bu.abs()                                     # |a shuffled pixel's channel|, |x| <= 4
    bound = (wl.abs().sum((2, 3)) @ per_mid.reshape(64, 4).max(1)[0] + bl.abs()).max() * c.out_scale + max(MEAN)
    assert float(fw.abs().sum((4, 5, 6)).max()) * 4.0 * c.out_scale <= float(bound)        # the fold's own sums obey the bound too
    assert_exact_domain(key, stored=[("x", c.x, torch.bfloat16), ("folded weights", fw, torch.bfloat16),
                                     ("folded bias", torch.stack([f[1] for f in folded]), torch.float32)],
                        absum=bound, unit=0.125, addends=[c.ref])
    return c
