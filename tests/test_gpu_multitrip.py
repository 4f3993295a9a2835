"""Kernel parity where the persistent tile loops take SEVERAL trips, through the C ABI (super_resolution_amd.ops).

The hot bf16 kernels run a fixed grid (about 256 workgroups times a few waves) that walks the tiles with a stride and a software
pipeline across trips: the next tile's operands are fetched under this tile's MFMAs (two and three tiles ahead in pw_kernel), loads
past the end are clamped to a valid tile, column sums and GAP partials are carried in registers from trip to trip.  Every launcher
caps the grid at the tile count, so at the shapes of test_gpu_ops.py / test_gpu_fp16_stream.py / test_gpu_hatx_ops.py (about 2 000
pixels at most) each wave or workgroup runs its loop body ONCE.  Here every case uses the smallest shape at which some loops take
>= 3 trips (>= 4 where the look-ahead is three deep) and others one trip fewer, on ragged frames (H, W no multiples of the tile,
H * W odd) and with B = 2 where the kernel indexes samples, so a flat-order tile straddles the sample boundary.

Assertions, per case:
  1. parity against a plain torch fp64 restatement on the same rounded operands, judged by helpers.check (the project's bars);
  2. for the pointwise kernels, BIT equality with the same kernel run over consecutive chunks that each fit inside one trip
     (a pixel's result depends on its own row only and its arithmetic order is fixed);
  3. the write footprint: outputs are pre-filled with NaN, everything the contract says is written is finite, pad channels keep
     their fill; pooled partial sums equal the pool of the stored map.
Each case asserts, from the named first-trip capacity below, that the trip counts it is meant to reach were reached; the launch
sites carry a comment that names the constant.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import _r8, check, conv_ref_banded, dev_randn, dev_rows, esc_weights_case, need_trips, q, rnd, run_chunked
from lattice import conv64r_trip_tiles

pytestmark = pytest.mark.gpu

# ---- tiles (pixels, blocks) the whole grid covers in ONE trip, as the launchers compute them -------------------------------------
# hat_pw.hip launch_pw_cfg: `int gx = 256 * wgs_per_cu;` workgroups of WAVES waves, one 16-pixel tile per wave, flat over B.
# launch_pw picks (wgs_per_cu, WAVES) from the LDS image: (3, 4) without residual operands when three images fit (144 -> 144 bf16:
# 46.7 KB), else (2, 4) or (1, 8)
PW_TRIP_TILES_3WG = 256 * 3 * 4     # 3072
PW_TRIP_TILES = 256 * 2 * 4         # 2048 (= 256 * 1 * 8)
# hat_mlp.hip hat_ocab_mlp / hat_ocab_qkv: `int gx = 256;` workgroups of nw = 8 waves, flat over B
MLP_TRIP_TILES = 256 * 8
QKV_TRIP_TILES = 256 * 8
# hat_pw.hip hat_aggr_cab: `int gx = 512 / (d.B < 2 ? 1 : 2);` workgroups of 4 waves PER SAMPLE (grid.y = B)
AGGR_CAB_TRIP_TILES = {1: 512 * 4, 2: 256 * 4}
# hat_pw.hip launch_tap3: `int gx = 256 * wgs_per_cu;` workgroups of 4 waves per sample; gx is what hat_conv3x3_small_groups returns
TAP3_WAVES = 4
# hat_esc13.hip hat_esc_conv13: `int gx = 256 / (B < 2 ? 1 : (B < 4 ? 2 : 4));` one 32 x 32 tile per workgroup, per sample
ESC13_TRIP_TILES = {1: 256, 2: 128}
ESC13_TILE = 32
# hat_misc.hip launch_ln: `dim3 grid(LN_BLOCKS, B)` with LN_BLOCKS = 1024 (hat_layernorm_blocks), 16 pixels per block and trip
LN_BLOCK_PIXELS = 16
# hat_misc.hip esc_weights_kernel: `for (int k0 = pp; k0 < nblk; k0 += np * 8 * 4)`, np = 1024 / (16 or 32 floats per GAP block)
ESCW_TRIP_BLOCKS = {16: 64 * 32, 32: 32 * 32}
CONV64R_TILE = 16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def nan_rows(B, N, ld, tdt, dev):
    return torch.full((B, N, ld), float("nan"), dtype=tdt, device=dev)


def bf16_round(x):
    return x.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------
# hat_linear (pw_kernel)
# ------------------------------------------------------------------------------------------------
LIN_GEOM = (2, 331, 301)      # 99 631 pixels per sample (odd), 12 454 tiles over both: 5 / 4 trips of 3072, 7 / 6 trips of 2048


@functools.lru_cache(maxsize=None)
def _lin_setup(cin: int, cout: int, dtype: str):
    """Packed weights, the input rows and the fp64 linear part (shared by the epilogues of one shape; never modified)."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = LIN_GEOM
    name = f"mt{cin}_{cout}"
    wgt = q(rnd(name + "w", (cout, cin), std=cin ** -0.5), dtype)
    bias = rnd(name + "b", (cout,), std=0.1)
    assert ops.linear_supported(cout, cin, dt)
    pw = ops.pack_linear_weight(wgt, bias, dt, dev)
    x = dev_rows(f"mtx{cin}", B, H * W, cin, _r8(cin), tdt, dev)
    lin = x[:, :, :cin].double() @ wgt.double().t().to(dev) + bias.double().to(dev)
    return pw, x, lin


def _lin_trip_check(pw, dtype, res: bool, cap: int):
    """The capacity the case names is the one launch_pw derives (restated from its LDS arithmetic), and the trip rule holds."""
    B, H, W = LIN_GEOM
    ks = pw.kpad // 32
    esize = 2 if dtype == "bf16" else 4
    lds = pw.nt * ks * 64 * 8 * esize + pw.nt * 16 * 4
    wgs = min(163840 // lds, 2 if res else 3)
    assert cap == (PW_TRIP_TILES_3WG if wgs == 3 else PW_TRIP_TILES), (pw.nt, ks, lds, wgs, cap)
    deep = not res and ks <= 5         # pw_kernel's DEEP copies: B operands three tiles ahead
    need_trips(-(-B * H * W // 16), cap, 4 if deep else 3, f"hat_linear nt {pw.nt} ks {ks}")
    return cap * 16


# name, Cin, Cout, dtype, first-trip tiles of the plain launch (residual launches are sized for two workgroups: 2048 always)
LIN_SHAPES = [
    ("aggr144", 144, 144, "bf16", PW_TRIP_TILES_3WG),   # DEEP, three workgroups per CU, pair stores
    ("kv288", 144, 288, "bf16", PW_TRIP_TILES),         # ONE slice of 18 n-tiles in bf16 (choose_nt_linear), eight waves, DEEP
    ("mlp2_288", 288, 144, "bf16", PW_TRIP_TILES),      # K > 160: not DEEP, eight waves
    ("lin180", 180, 180, "bf16", PW_TRIP_TILES),        # partial last n-tile (tail_ok)
    ("kv360", 180, 360, "bf16", PW_TRIP_TILES),         # 23 n-tiles, partial last one
    ("aggr144_f32", 144, 144, "f32", PW_TRIP_TILES),
    ("lin180_f32", 180, 180, "f32", PW_TRIP_TILES),
]


@pytest.mark.parametrize("case", LIN_SHAPES, ids=[c[0] for c in LIN_SHAPES])
def test_linear_gelu_rows_multitrip(case):
    """Plain + GELU to T rows (no residual operands: the DEEP copies where K <= 160)."""
    name, cin, cout, dtype, cap = case
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = LIN_GEOM
    N = H * W
    pw, x, lin = _lin_setup(cin, cout, dtype)
    chunk = _lin_trip_check(pw, dtype, False, cap)
    ldx, ldo = _r8(cin), _r8(cout)
    out = nan_rows(B, N, ldo, tdt, dev)
    ops.linear(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=ldx, ldo=ldo, act=ops.ACT_GELU)
    torch.cuda.synchronize()
    ref = F.gelu(lin)
    check(out[:, :, :cout].float(), bf16_round(ref) if dtype == "bf16" else ref, dtype, name + " gelu")
    if ldo > cout:
        assert torch.isnan(out[:, :, cout:].float()).all(), "pad channels past n_store keep their fill"
    out2 = nan_rows(B, N, ldo, tdt, dev)
    run_chunked(lambda v, b: ops.linear(pw, v["x"], v["out"], B=1, H=1, W=v["x"].shape[1], dtype=dt, ldx=ldx, ldo=ldo, act=ops.ACT_GELU),
                dict(x=x, out=out2), B, N, chunk)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :, :cout], out2[:, :, :cout]), f"{name}: the multi-trip launch differs from its one-trip chunks"


RES_SHAPES = [c for c in LIN_SHAPES if c[2] in (144, 180)]


@pytest.mark.parametrize("case", RES_SHAPES, ids=[c[0] for c in RES_SHAPES])
def test_linear_residual_scaled_r2_multitrip(case):
    """fp32 residual in place + the scaled T residual (per-sample scale table in LDS) + a split source for the first 16 channels:
    the ESC aggregation's launch."""
    name, cin, cout, dtype, _ = case
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = LIN_GEOM
    N = H * W
    pw, x, _ = _lin_setup(cin, cout, dtype)
    chunk = _lin_trip_check(pw, dtype, True, PW_TRIP_TILES)
    ldx, ldo, cs = _r8(cin), _r8(cout), 16
    x0 = dev_rows(name + "x0", B, N, cs, cs, tdt, dev)
    r1 = dev_randn(name + "r1", (B, N, cout), dev)
    r2 = dev_rows(name + "r2", B, N, cout, ldo, tdt, dev)
    sc = rnd(name + "sc", (B, cout), std=0.3)
    scd = torch.zeros(B, pw.npad, device=dev)
    scd[:, :cout] = sc.to(dev)
    wgt = q(rnd(f"mt{cin}_{cout}w", (cout, cin), std=cin ** -0.5), dtype).double().to(dev)
    bias = rnd(f"mt{cin}_{cout}b", (cout,), std=0.1).double().to(dev)
    xin = torch.cat([x0.double(), x[:, :, cs:cin].double()], -1)
    ref = xin @ wgt.t() + bias + r1.double() + sc.double().to(dev)[:, None, :] * r2[:, :, :cout].double()

    def launch(v, b, B_, H_, W_):
        ops.linear(pw, v["x"], v["out"], B=B_, H=H_, W=W_, dtype=dt, ldx=ldx, ldo=cout, out_mode=ops.O_NHWC_F32, x0=v["x0"], c_split=cs,
                   ldx0=cs, r1=v["out"], ldr1=cout, r2=v["r2"], ldr2=ldo, r2scale=(scd if b is None else scd[b:b + 1]), r2scale_bstride=pw.npad)

    out = r1.clone()
    launch(dict(x=x, x0=x0, r2=r2, out=out), None, B, H, W)
    torch.cuda.synchronize()
    check(out, ref, dtype, name + " residual epilogue", f32_tol=3e-5)
    out2 = r1.clone()
    run_chunked(lambda v, b: launch(v, b, 1, 1, v["x"].shape[1]), dict(x=x, x0=x0, r2=r2, out=out2), B, N, chunk)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), f"{name}: the multi-trip launch differs from its one-trip chunks"


LN_SHAPES = [c for c in LIN_SHAPES if c[2] in (144, 180) and c[3] == "bf16"]


@pytest.mark.parametrize("case", LN_SHAPES, ids=[c[0] for c in LN_SHAPES])
def test_linear_residual_fused_layernorm_multitrip(case):
    """fp32 residual in place (r1 only) with the consumer's LayerNorm fused behind it: the OCAB projection / MLP fc2 launch."""
    name, cin, cout, dtype, _ = case
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = LIN_GEOM
    N = H * W
    pw, x, lin = _lin_setup(cin, cout, dtype)
    chunk = _lin_trip_check(pw, dtype, True, PW_TRIP_TILES)
    ldx, ldo = _r8(cin), _r8(cout)
    r1 = dev_randn(name + "lr1", (B, N, cout), dev)
    g_, b_ = (1 + rnd(name + "lg", (cout,), std=0.1)).to(dev), rnd(name + "lb", (cout,), std=0.1).to(dev)
    ref = lin + r1.double()
    ref_ln = F.layer_norm(ref, (cout,), g_.double(), b_.double(), 1e-5)

    def launch(v, B_, H_, W_):
        ops.linear(pw, v["x"], v["out"], B=B_, H=H_, W=W_, dtype=dt, ldx=ldx, ldo=cout, out_mode=ops.O_NHWC_F32, r1=v["out"], ldr1=cout,
                   ln=(g_, b_), ln_out=v["ln"], ld_ln=ldo)

    out, lno = r1.clone(), nan_rows(B, N, ldo, tdt, dev)
    launch(dict(x=x, out=out, ln=lno), B, H, W)
    torch.cuda.synchronize()
    check(out, ref, dtype, name + " residual epilogue", f32_tol=3e-5)
    check(lno[:, :, :cout].float(), ref_ln, dtype, name + " fused LayerNorm", f32_tol=5e-5)
    if ldo > cout:
        assert torch.isnan(lno[:, :, cout:].float()).all(), "pad channels of the LayerNorm rows keep their fill"
    out2, lno2 = r1.clone(), nan_rows(B, N, ldo, tdt, dev)
    run_chunked(lambda v, b: launch(v, 1, 1, v["x"].shape[1]), dict(x=x, out=out2, ln=lno2), B, N, chunk)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), f"{name}: the multi-trip launch differs from its one-trip chunks"
    assert torch.equal(lno[:, :, :cout], lno2[:, :, :cout]), f"{name}: fused LayerNorm rows differ from the one-trip chunks"


@pytest.mark.parametrize("halves", [(True, False), (False, True), (True, True)], ids=["r1_fp16", "out_fp16", "inplace_fp16"])
@pytest.mark.parametrize("variant", ["ln16", "ln_ld148", "no_ln"])
def test_ocab_proj_fp16_stream_multitrip(variant, halves):
    """The FP16-row copies of the OCAB projection (144 -> 144, hat_linear's reserved0 bits; test_gpu_fp16_stream.py's variants):
    r1 as FP16 rows, the fp32 result stored as FP16 rows, and both in place as the engine runs it."""
    dev, ops = _dev(), _ops()
    dt, C = ops.HAT_BF16, 144
    B, H, W = LIN_GEOM
    N = H * W
    pw, x, lin = _lin_setup(C, C, "bf16")
    chunk = _lin_trip_check(pw, "bf16", True, PW_TRIP_TILES)
    r_half, o_half = halves
    inplace = r_half and o_half
    r16 = dev_randn("p16r", (B, N, C), dev, std=1.5, mean=0.3).half()
    ldn = 148 if variant == "ln_ld148" else C
    g_, b_ = (1 + rnd("p16g", (C,), std=0.1)).to(dev), rnd("p16b", (C,), std=0.1).to(dev)
    ref = lin + r16.double()
    ref_ln = F.layer_norm(ref, (C,), g_.double(), b_.double(), 1e-5)

    def launch(v, B_, H_, W_):
        lnkw = dict(ln=(g_, b_), ln_out=v["ln"], ld_ln=ldn) if variant != "no_ln" else {}
        ops.linear(pw, v["x"], v["out"], B=B_, H=H_, W=W_, dtype=dt, ldx=C, ldo=C, out_mode=ops.O_NHWC_F32, r1=v["r1"], ldr1=C, **lnkw)

    def buffers():
        r1 = r16.clone() if r_half else r16.float()
        out = r1 if inplace else nan_rows(B, N, C, torch.float16 if o_half else torch.float32, dev)
        return dict(x=x, r1=r1, out=out, ln=nan_rows(B, N, ldn, torch.bfloat16, dev))

    big = buffers()
    launch(big, B, H, W)
    torch.cuda.synchronize()
    check(big["out"].float(), ref, "bf16", f"projection {variant} {halves}")
    if variant != "no_ln":
        check(big["ln"][:, :, :C].float(), ref_ln, "bf16", f"projection {variant} {halves} fused LayerNorm")
        if ldn > C:
            assert torch.isnan(big["ln"][:, :, C:].float()).all(), "pad channels of the LayerNorm rows keep their fill"
    parts = buffers()
    run_chunked(lambda v, b: launch(v, 1, 1, v["x"].shape[1]), parts, B, N, chunk)
    torch.cuda.synchronize()
    assert torch.equal(big["out"], parts["out"]), f"{variant} {halves}: the multi-trip launch differs from its one-trip chunks"
    if variant != "no_ln":
        assert torch.equal(big["ln"][:, :, :C], parts["ln"][:, :, :C]), f"{variant} {halves}: fused LayerNorm rows differ"


# ------------------------------------------------------------------------------------------------
# hat_ocab_mlp / hat_ocab_qkv
# ------------------------------------------------------------------------------------------------
MLP_GEOM = (2, 229, 229)      # 52 441 pixels per sample (odd), 6 556 tiles over both: 4 / 3 trips of 2048


@functools.lru_cache(maxsize=None)
def _mlp_setup():
    dev, ops = _dev(), _ops()
    B, H, W = MLP_GEOM
    C, hid = 144, 288
    w1, b1 = q(rnd("mmw1", (hid, C), std=C ** -0.5), "bf16"), rnd("mmb1", (hid,), std=0.2)
    w2, b2 = q(rnd("mmw2", (C, hid), std=hid ** -0.5), "bf16"), rnd("mmb2", (C,), std=0.2)
    pm = ops.pack_ocab_mlp(w1, b1, w2, b2, dev)
    x = dev_rows("mmx", B, H * W, C, C, torch.bfloat16, dev)
    hdn = F.gelu(x.double() @ w1.double().t().to(dev) + b1.double().to(dev))
    upd = hdn @ w2.double().t().to(dev) + b2.double().to(dev)
    return pm, x, upd


@pytest.mark.parametrize("mode", ["f32_inplace", "rows", "rows_r1_fp16"])
def test_ocab_mlp_multitrip(mode):
    """hat_ocab_mlp: fp32 out in place over r1, T rows out, T rows out with r1 as FP16 rows."""
    dev, ops = _dev(), _ops()
    B, H, W = MLP_GEOM
    N, C = H * W, 144
    need_trips(-(-B * N // 16), MLP_TRIP_TILES, 3, "hat_ocab_mlp")
    pm, x, upd = _mlp_setup()
    r1 = dev_randn("mmr1", (B, N, C), dev, std=1.5, mean=0.3)
    r1 = r1.half() if mode == "rows_r1_fp16" else r1
    ref = r1.double() + upd

    def launch(v, B_, H_, W_):
        ops.ocab_mlp(pm, v["x"], v["r1"], v["out"], B=B_, H=H_, W=W_, ldx=C, ldr1=C, ldo=C, out_f32=(mode == "f32_inplace"), dtype=ops.HAT_BF16)

    def buffers():
        r = r1.clone()
        return dict(x=x, r1=r, out=(r if mode == "f32_inplace" else nan_rows(B, N, C, torch.bfloat16, dev)))

    big = buffers()
    launch(big, B, H, W)
    torch.cuda.synchronize()
    check(big["out"].float(), ref, "bf16", f"fused OCAB MLP ({mode})")
    parts = buffers()
    run_chunked(lambda v, b: launch(v, 1, 1, v["x"].shape[1]), parts, B, N, MLP_TRIP_TILES * 16)
    torch.cuda.synchronize()
    assert torch.equal(big["out"], parts["out"]), f"hat_ocab_mlp ({mode}): the multi-trip launch differs from its one-trip chunks"


def test_ocab_qkv_multitrip():
    """hat_ocab_qkv: [q * d^-0.5 | k | v] rows of 432 channels."""
    dev, ops = _dev(), _ops()
    B, H, W = MLP_GEOM
    N, C = H * W, 144
    need_trips(-(-B * N // 16), QKV_TRIP_TILES, 3, "hat_ocab_qkv")
    x = _mlp_setup()[1]
    wq, bq = rnd("mqw", (C, C), std=C ** -0.5), rnd("mqb", (C,), std=0.2)
    wkv, bkv = rnd("mkvw", (2 * C, C), std=C ** -0.5), rnd("mkvb", (2 * C,), std=0.2)
    sc = 24 ** -0.5
    wall = torch.cat([q(wq * sc, "bf16"), q(wkv, "bf16")], 0).double().to(dev)
    ref = x.double() @ wall.t() + torch.cat([bq * sc, bkv]).double().to(dev)
    pm = ops.pack_ocab_qkv(wq, bq, wkv, bkv, sc, dev)
    out = nan_rows(B, N, 432, torch.bfloat16, dev)
    ops.ocab_qkv(pm, x, out, B=B, H=H, W=W, ldx=C, ldo=432, dtype=ops.HAT_BF16)
    torch.cuda.synchronize()
    check(out.float(), ref, "bf16", "fused q / kv projection")
    out2 = nan_rows(B, N, 432, torch.bfloat16, dev)
    run_chunked(lambda v, b: ops.ocab_qkv(pm, v["x"], v["out"], B=1, H=1, W=v["x"].shape[1], ldx=C, ldo=432, dtype=ops.HAT_BF16),
                dict(x=x, out=out2), B, N, QKV_TRIP_TILES * 16)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "hat_ocab_qkv: the multi-trip launch differs from its one-trip chunks"


# ------------------------------------------------------------------------------------------------
# hat_aggr_cab (through hat_cab_fold, as test_gpu_ops.test_aggr_with_folded_cab)
# ------------------------------------------------------------------------------------------------
def test_aggr_with_folded_cab_multitrip():
    """x = t + aggr([x0 | n[16:]]) + conv_scale * ECA(c2) * c2, c2 = conv3x3(c1) + b2 folded into the GEMM as three k-steps of
    gathered neighbours: one grid row per sample, 3 278 tiles on 1 024 waves."""
    B, H, W = 2, 229, 229
    C, mid, dtype = 144, 6, "bf16"
    dev, ops = _dev(), _ops()
    dt, tdt, N = ops.DTYPE_CODE[dtype], torch.bfloat16, H * W
    need_trips(-(-N // 16), AGGR_CAB_TRIP_TILES[B], 3, "hat_aggr_cab")
    x = dev_rows("macx", B, N, C, C, tdt, dev)
    x0 = dev_rows("macx0", B, N, 16, 16, tdt, dev)
    c1d = torch.zeros(B, N, 8, dtype=tdt, device=dev)
    c1d[:, :, :mid] = F.gelu(dev_randn("macc1", (B, N, mid), dev)).to(tdt)
    t = dev_randn("mact", (B, N, C), dev)
    wa, ba = q(rnd("macwa", (C, C), std=C ** -0.5), dtype), rnd("macba", (C,), std=0.1)
    w2, b2 = rnd("macw2", (C, mid, 3, 3), std=(9 * mid) ** -0.5), rnd("macb2", (C,), std=0.1)
    wk = rnd("macwk", (5,), std=1.0)
    conv_scale = 0.37
    c2 = conv_ref_banded(c1d[:, :, :mid].reshape(B, H, W, mid), w2, b2).reshape(B, N, C)
    e = torch.sigmoid(F.conv1d(c2.mean(1)[:, None, :], wk.double().to(dev)[None, None, :], padding=2))[:, 0]      # (B, C)
    xin = torch.cat([x0.double(), x[:, :, 16:].double()], -1)
    ref = t.double() + xin @ wa.double().t().to(dev) + ba.double().to(dev) + conv_scale * e[:, None, :] * c2
    pw = ops.pack_linear_weight(wa, ba, dt, dev)
    colsum = torch.zeros(B, 1, 16, device=dev)
    colsum[:, 0, :8] = c1d.float().sum(1)
    scale = torch.zeros(B, pw.npad, device=dev)
    wf = torch.zeros(B, pw.nt * 3 * 512, dtype=tdt, device=dev)
    bias_b = torch.zeros(B, pw.npad, device=dev)
    ops.cab_fold(c1d, colsum, 1, 16, w2.to(dev).contiguous(), b2.to(dev), wk.to(dev), 5, ba.to(dev), conv_scale, scale, wf, bias_b,
                 torch.zeros(B, 32, 16, device=dev), B=B, H=H, W=W, C_=C, mid=mid, dtype=dt)
    out = nan_rows(B, N, C, torch.float32, dev)
    ops.aggr_cab(pw, x, out, c1d, wf, bias_b, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, x0=x0, c_split=16, ldx0=16, r1=t, ldr1=C)
    torch.cuda.synchronize()
    check(out, ref, dtype, "aggr + folded cab")


# ------------------------------------------------------------------------------------------------
# hat_conv3x3_small (tap3_kernel): column sums carried across trips
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [("cab0", 144, 6, 1), ("cab2", 6, 144, 0)], ids=lambda c: c[0])
def test_conv3x3_small_multitrip(case, dtype):
    """144 -> 6 with GELU and 6 -> 144, with column sums; a wave's sums now add up over its trips."""
    name, Cin, Cout, act = case
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    if not ops.conv3x3_small_supported(Cout, Cin, dt):
        pytest.skip("weight slice does not fit half the LDS in this dtype (the engine uses hat_conv)")
    B, H, W = 2, 331, 301       # 6 227 tiles per sample: 3 / 2 trips of 768 x 4 waves, 4 / 3 trips of 512 x 4
    N = H * W
    wgt = q(rnd("m3" + name + "w", (Cout, Cin, 3, 3), std=(9 * Cin) ** -0.5), dtype)
    bias = rnd("m3" + name + "b", (Cout,), std=0.1)
    pw = ops.pack_linear_weight(wgt, bias, dt, dev)
    groups = ops.conv3x3_small_groups(pw, B, H, W, dt)
    need_trips(-(-N // 16), groups * TAP3_WAVES, 3, "hat_conv3x3_small")
    ldx, ldo, n_store = _r8(Cin), _r8(Cout), (Cout + 3) // 4 * 4
    x = dev_rows("m3" + name + "x", B, N, Cin, ldx, tdt, dev)
    ref = conv_ref_banded(x[:, :, :Cin].reshape(B, H, W, Cin), wgt, bias)
    ref = (F.gelu(ref) if act else ref).reshape(B, N, Cout)
    out = nan_rows(B, N, ldo, tdt, dev)
    colsum = torch.full((B, groups, pw.npad), float("nan"), device=dev)
    ops.conv3x3_small(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=ldx, ldo=ldo, act=act, n_store=n_store, colsum=colsum)
    torch.cuda.synchronize()
    check(out[:, :, :Cout].float(), bf16_round(ref) if dtype == "bf16" else ref, dtype, name)
    if ldo > n_store:
        assert torch.isnan(out[:, :, n_store:].float()).all(), "pad channels past n_store keep their fill"
    assert torch.isfinite(colsum).all()
    pooled = colsum.double().sum(1)[:, :Cout] / N
    check(pooled, ref.mean(1), dtype, name + " column sums", f32_tol=3e-5)
    check(pooled, out[:, :, :Cout].double().mean(1), "f32", name + " column sums = pool of the stored map", f32_tol=1e-5)


# ------------------------------------------------------------------------------------------------
# hat_conv -> conv64r_kernel (the Upsample convs and the 64 -> 64 conv before them)
# ------------------------------------------------------------------------------------------------
CONV64R_CASES = [
    # name, B, H, W, r (0: 64 -> 64 NHWC rows with LeakyReLU), trips wanted
    ("r2_B2_121x140", 2, 121, 140, 2, 3),      # 4 slices, nwps 64, 144 tiles: 3 / 2 trips, tiles straddle the sample boundary
    ("r3_100x120", 1, 100, 120, 3, 3),         # 9 slices, nwps 24, 56 tiles: 3 / 2 trips
    ("c64_lrelu_B2_260x250", 2, 260, 250, 0, 3),   # 1 slice, nwps 256, 544 tiles: 3 / 2 trips
    ("r2_shrunk_m_64x80", 1, 64, 80, 2, 0),    # 20 tiles: m shrinks 8 -> 3, nwps 24: workgroups wgi >= 20 return at once with m > 1
]


@pytest.mark.parametrize("case", CONV64R_CASES, ids=[c[0] for c in CONV64R_CASES])
def test_conv64r_multitrip(case):
    name, B, H, W, r, depth = case
    dev, ops = _dev(), _ops()
    dt, tdt = ops.HAT_BF16, torch.bfloat16
    cout = 64 * r * r if r else 64
    wgt = q(rnd("m64w" + name, (cout, 64, 3, 3), std=576 ** -0.5), "bf16")
    bias = rnd("m64b" + name, (cout,), std=0.1)
    perm = None
    if r:
        n = torch.arange(cout)
        perm = (n % 64) * (r * r) + n // 64
    pw = ops.pack_conv_weight(wgt, bias, dt, dev, out_perm=perm)
    # what hat_conv64r_can_launch asks of the packed layer (bf16, 3 x 3, 64 inputs, whole 64-channel slices, every channel stored)
    assert pw.cin == 64 and pw.ksize == 3 and pw.npad == cout and cout % 64 == 0 and pw.kpad >= 576
    nsl = cout // 64
    ntiles = -(-H // CONV64R_TILE) * -(-W // CONV64R_TILE) * B
    nwps, m = conv64r_trip_tiles(nsl, ntiles)
    if depth:
        assert m == max(32 // nsl, 1)
        need_trips(ntiles, nwps, depth, "conv64r_kernel")
    else:
        assert 1 < m < 32 // nsl and ntiles < nwps, (m, nwps, ntiles)     # shrunk m, idle workgroups behind the last tile
    x = dev_rows("m64x" + name, B, H * W, 64, 64, tdt, dev)
    ref = conv_ref_banded(x.reshape(B, H, W, 64), wgt, bias)
    if r:
        ref = F.pixel_shuffle(ref.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
        out = nan_rows(B, H * r * W * r, 64, tdt, dev)
        ops.conv(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=64, ldo=64, out_mode=ops.O_PIXSHUF_T, ps_r=r)
        got = out.float().reshape(B, H * r, W * r, 64)
    else:
        ref = F.leaky_relu(ref, 0.01)
        out = nan_rows(B, H * W, 64, tdt, dev)
        ops.conv(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=64, ldo=64, act=2)
        got = out.float().reshape(B, H, W, 64)
    torch.cuda.synchronize()
    check(got, bf16_round(ref), "bf16", name)


# ------------------------------------------------------------------------------------------------
# hat_esc_conv13
# ------------------------------------------------------------------------------------------------
def test_esc_conv13_multitrip():
    """13 x 13, 16 -> 16 with per-sample weights on 0.5 Mpx: 272 tiles of 32 x 32 per sample on 128 workgroups (3 / 2 trips), the
    next tile's haloed input fetched under the K loop, ragged right and bottom tiles."""
    B, H, W = 2, 530, 500
    dev, ops = _dev(), _ops()
    dt = ops.HAT_BF16
    C, pd, ks = 144, 16, 13
    need_trips(-(-H // ESC13_TILE) * -(-W // ESC13_TILE), ESC13_TRIP_TILES[B], 3, "hat_esc_conv13")
    x = torch.zeros(B, H * W, C, dtype=torch.bfloat16, device=dev)       # rows of 144 channels, the conv reads the first 16
    x[:, :, :pd] = dev_randn("me13x", (B, H * W, pd), dev).to(torch.bfloat16)
    x[:, :, pd:] = 1.0e4                                                   # (nothing beyond them may leak in)
    wt = q(rnd("me13w", (B, pd, pd, ks, ks), std=(pd * ks * ks) ** -0.5), "bf16")          # [b][co][ci][ty][tx]
    ref = conv_ref_banded(x[:, :, :pd].reshape(B, H, W, pd), wt, band=128)
    kc = ops.KC[dt] * 3
    kpad = -(-(ks * ks * pd) // kc) * kc
    wp = torch.zeros(B, 16, kpad)
    wp[:, :pd, :ks * ks * pd] = wt.permute(0, 1, 3, 4, 2).reshape(B, pd, ks * ks * pd)     # K = tap * 16 + ci
    y = nan_rows(B, H * W, 16, torch.bfloat16, dev)
    ops.esc_conv13(x, wp.to(torch.bfloat16).to(dev).contiguous(), y, B=B, H=H, W=W, ldx=C, kpad=kpad, dtype=dt)
    torch.cuda.synchronize()
    check(y.reshape(B, H, W, 16).float(), ref, "bf16", "esc conv13 vs fp64")


# ------------------------------------------------------------------------------------------------
# hat_layernorm (ln_kernel): GAP partials carried across trips
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [144, 180])
def test_layernorm_multitrip(C):
    """52 441 pixels per sample on 1024 blocks x 16 pixels: blocks 0..205 take 4 trips, the rest 3; T rows with GAP partials (16
    pooled channels at C = 144, 24 at C = 180: blocks of 32 floats) and the fp32-output launch."""
    dev, ops = _dev(), _ops()
    dt, tdt = ops.HAT_BF16, torch.bfloat16
    B, N = 2, 229 * 229
    nblk = ops.layernorm_blocks()
    need_trips(N, nblk * LN_BLOCK_PIXELS, 3, "hat_layernorm")
    x = dev_randn(f"mlnx{C}", (B, N, C), dev, std=2.0, mean=0.5)
    gm, bt = (1 + rnd("mlng", (C,), std=0.1)).to(dev), rnd("mlnb", (C,), std=0.1).to(dev)
    ref = F.layer_norm(x.double(), (C,), gm.double(), bt.double(), 1e-5)
    ld = _r8(C)
    gap_c = {144: 16, 180: 24}[C]
    y = nan_rows(B, N, ld, tdt, dev)
    gap = torch.full((B, nblk, 32 if gap_c > 16 else 16), float("nan"), device=dev)
    ops.layernorm(x, y, gm, bt, B=B, npix=N, C_=C, ldy=ld, out_f32=False, dtype=dt, gap=gap, gap_c=gap_c)
    yf = nan_rows(B, N, C, torch.float32, dev)
    ops.layernorm(x, yf, gm, bt, B=B, npix=N, C_=C, ldy=C, out_f32=True, dtype=dt)
    torch.cuda.synchronize()
    check(y[:, :, :C].float(), ref, "bf16", "layernorm -> T")
    check(yf, ref, "f32", "layernorm -> fp32")
    if ld > C:
        assert torch.isnan(y[:, :, C:].float()).all(), "pad channels of the rows keep their fill"
    assert torch.isfinite(gap).all() and bool((gap[:, :, gap_c:] == 0).all())      # (the dead floats of a 32-float block are zeros)
    pooled = gap.double().sum(1)[:, :gap_c] / N
    check(pooled, y[:, :, :gap_c].double().mean(1), "f32", "gap partial sums = pool of the stored map", f32_tol=1e-5)
    check(pooled, ref[:, :, :gap_c].mean(1), "f32", "gap partial sums vs the unrounded LayerNorm", f32_tol=1e-3)


# ------------------------------------------------------------------------------------------------
# hat_esc_weights: the reduction over the GAP partial blocks of a large frame
# ------------------------------------------------------------------------------------------------
ESCW_CASES = [(16, 13, 2049), (16, 13, 7200), (24, 15, 1025), (24, 15, 3000), (32, 17, 1025), (32, 17, 3000)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("pdim,ks,nblk", ESCW_CASES)
def test_esc_weights_multitrip(dtype, pdim, ks, nblk):
    """One block past the first iteration of the reduction loop (its second iteration reads a single live block and 31 clamped
    ones per thread), and a 720p frame's 7 200 blocks (four iterations; three at the 32-float layout of pdim > 16)."""
    dev, ops = _dev(), _ops()
    cap = ESCW_TRIP_BLOCKS[16 if pdim <= 16 else 32]
    assert nblk > cap and (nblk == cap + 1 or nblk > 2 * cap), (nblk, cap)
    got, weff, wout, npad = esc_weights_case(ops, dev, dtype, pdim, ks, nblk)
    check(got, weff, dtype, "esc weights", f32_tol=1e-5)
    assert torch.isfinite(wout.float()).all()
    if pdim < npad:
        assert float(wout[:, pdim:].float().abs().max()) == 0.0
