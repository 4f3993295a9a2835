"""GPU parity tests, per kernel, through the C ABI (super_resolution_amd.ops) for the four entries the HATX variant and the
band-sharded forward depend on: hat_ocab_keybias, hat_ocab_attention_kb, hat_sgfn_gate, hat_add_f32 — each against a plain fp64
restatement on the kernel's own inputs (helpers.ref_*, pinned to the oracle by test_hatx_ops_ref_cpu.py).

Tolerances are test_gpu_ops.py's: helpers.check (fp32: max-abs <= 2e-5 * scale, 5e-5 for the attention core as in
test_ocab_attention; bf16: relative L2 <= 1.2e-2 and max-abs <= 6e-2 * scale).

The ranking tests need a WELL DEFINED kept set, so their inputs are constructed and an assert on the inputs proves, before the
kernel runs, that in every window the scores on either side of the k_keep boundary are either an exact tie of the inputs
(decided by the lowest-key-index rule) or differ by >= SEP = 1e-4 relative:
  norm mode   the fp32 sum of C <= 180 squares is off by at most about (C + 2) * 2^-24 ~ 1.1e-5 relative, sqrtf adds 2^-24;
  focus mode  tanhf is good to a few ulp (2^-24 relative each), the reference score is float32(tanh_fp64(sal)).
No test here feeds a NaN score (include/hat_mi355x.h says what the kernel does with one).
"""
import pytest
import torch

from oracle import hat_oracle as O
from helpers import _r8, check, key_windows, q, ref_attention_kb, ref_keybias, ref_sgfn_gate, rnd, to_dev

pytestmark = pytest.mark.gpu

DT = ["f32", "bf16"]
SEP = 1e-4
NINF = float("-inf")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def _perm(seed, n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------
# hat_ocab_keybias
# ------------------------------------------------------------------------------------------------
KB_WINDOWS = [(16, 24, 144), (8, 12, 24), (16, 25, 180), (8, 13, 48)]          # ws, wse, key channels
KB_MODES = [("focus", "f32", 8), ("focus", "bf16", 8), ("focus", "bf16", -8), ("norm", "f32", 0), ("norm", "bf16", 0)]
KB_MODE_IDS = ["focus_f32", "focus_bf16", "focus_f32sal_bf16kv", "norm_f32", "norm_bf16"]


def focus_map(seed, B, H, W, sal_dtype, lo=-3.0, hi=3.0):
    """A seeded permutation of a 400-point grid on [lo, hi] (|sal| <= 4: far from where tanhf's last ulp could reorder distinct
    inputs), rounded to the storage type.  Grid points repeat, and bf16 rounding merges more: those are EXACT ties."""
    n = B * H * W
    grid = torch.linspace(lo, hi, 400, dtype=torch.float64)[torch.arange(n) % 400]
    return q(grid[_perm(seed, n)].reshape(B, H, W).float(), sal_dtype)


def norm_keys(seed, B, H, W, C, dtype):
    """Key vectors whose L2 norms are a seeded permutation of the grid 1 + i * 1e-3 (different content per sample): a random
    direction scaled to that norm and rounded to the storage type.  Rounding C bf16 channels moves a squared norm by about
    +-0.25 / C of itself, more than the grid step, so channel 0 is held back as a trim: the direction takes 1 - 0.45 / C of the
    squared norm and channel 0 = sqrt(what the rounded channels leave); its own rounding (2^-8 relative) moves the norm by
    2^-8 of that small share only.  assert_separated() has the last word on what the kernel is asked to rank."""
    n = B * H * W
    share = 0.45 / C
    t = (1.0 + 1e-3 * torch.arange(n, dtype=torch.float64))[_perm(seed, n)]
    u = rnd(f"kdir{seed}", (n, C)).double()
    u[:, 0] = 0.0
    x = q((u / u.norm(dim=1, keepdim=True) * (t * (1 - share) ** 0.5)[:, None]).float(), dtype)
    left = t ** 2 - x.double().pow(2).sum(1)
    assert (left > 0).all() and (left < 2 * share * t ** 2).all()
    x[:, 0] = q(left.sqrt().float(), dtype)
    assert ((x.double().norm(dim=1) - t).abs() <= 2.0 ** -8 * 2 * share * t).all(), "the constructed norms miss their grid"
    return x.reshape(B, H, W, C)


def assert_separated(score, salw, k_keep):
    """score (B,nWy,nWx,nk): the fp64 reference scores; salw: the saliency value behind each (0 for a padded key), or None in
    norm mode.  Returns how many windows' boundaries are exact ties."""
    nk = score.shape[-1]
    if k_keep >= nk:
        return 0
    order = torch.argsort(-score, dim=-1, stable=True)[..., k_keep - 1:k_keep + 1]
    a, b = torch.gather(score, -1, order).unbind(-1)
    apart = (a > b) & ((a - b) >= SEP * torch.maximum(a.abs(), b.abs()))
    if salw is None:
        tie = (a == 0) & (b == 0)                                  # zero-padded keys only: in-image norms are >= 1
    else:
        sa, sb = torch.gather(salw.double(), -1, order).unbind(-1)
        tie = (a == b) & ((sa == sb) | ((sa >= 20) & (sb >= 20)))  # equal inputs, or tanh saturated to exactly 1 in fp32 AND fp64
    assert (apart | tie).all(), f"the inputs leave the kept set of {int((~(apart | tie)).sum())} windows undefined (k_keep {k_keep})"
    return int(tie.sum())


def run_keybias(sal, ldsal, k, ws, wse, k_keep, dtype):
    """Launch hat_ocab_keybias on kv = [k | garbage v] with a NaN-filled kb; returns kb on the host."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W, C = k.shape
    nkp = (wse * wse + 15) // 16 * 16
    kvd = to_dev(torch.cat([k, torch.full_like(k, 77.0)], -1), _r8(2 * C), tdt, dev)
    sd = None
    if sal is not None:
        sd = torch.full((B, H * W, abs(ldsal)), 55.0, dtype=torch.float32 if ldsal < 0 else tdt, device=dev)   # channel 0 = the map
        sd[:, :, 0] = sal.reshape(B, H * W).to(dev).to(sd.dtype)
    kb = torch.full((B, H // ws, W // ws, nkp), float("nan"), device=dev)
    ops.ocab_keybias(sd, kvd, kb, B=B, H=H, W=W, C_=C, ws=ws, wse=wse, pad=(wse - ws + 1) // 2, k_keep=k_keep, ldsal=ldsal,
                     ldkv=_r8(2 * C), dtype=dt)
    torch.cuda.synchronize()
    return kb.cpu()


def check_keybias(got, sal, k, ws, wse, k_keep, what):
    """Every assertion of the issue on one launch; the inputs' separation is asserted first.  Returns the tie count."""
    nk, pad = wse * wse, (wse - ws + 1) // 2
    focus = sal is not None
    kb, keep = ref_keybias(sal, k, ws, wse, pad, k_keep, score_dtype=torch.float32)
    if focus:
        salw = key_windows(sal.double(), ws, wse, pad)[0]
        ties = assert_separated(torch.tanh(salw).float().double(), salw, k_keep)
    else:
        ties = assert_separated(key_windows(k.double(), ws, wse, pad)[0].pow(2).sum(-1).sqrt(), None, k_keep)
    what = f"{what} k_keep {k_keep}"
    assert got.shape == kb.shape, what
    assert not torch.isnan(got).any(), what + ": a NaN of the pre-filled buffer survived"
    finite = torch.isfinite(got[..., :nk])
    assert (finite.sum(-1) == min(k_keep, nk)).all(), what + f": kept counts {sorted(set(finite.sum(-1).flatten().tolist()))}"
    wrong = finite != keep
    assert not wrong.any(), what + f": kept set differs in {int(wrong.any(-1).sum())} windows, first at {wrong.nonzero()[0].tolist()}"
    assert (got[..., :nk][~keep] == NINF).all(), what + ": a pruned key is not -inf"
    assert (got[..., nk:] == 0).all(), what + ": dead tail"
    if focus:
        check(got[..., :nk][keep], kb[..., :nk][keep], "f32", what + ": kept values")
    else:
        assert (got[..., :nk][keep] == 0).all(), what + ": kept values are exactly 0 without a focus head"
    return ties


def _keeps(nk):
    return [1, int(0.6 * nk), nk - 1, nk, nk + 5]


@pytest.mark.parametrize("mode", KB_MODES, ids=KB_MODE_IDS)
@pytest.mark.parametrize("win", KB_WINDOWS, ids=[f"ws{w[0]}_wse{w[1]}" for w in KB_WINDOWS])
def test_keybias(win, mode):
    """B = 2 with different content per sample, 4 x 3 windows (interior windows, four edges, four corners), every k_keep of the
    issue.  focus_f32sal_bf16kv is the engine's bf16 call: the saliency map is fp32 (ldsal = -8), kv is bf16."""
    (ws, wse, C), (kind, dtype, ldsal) = win, mode
    B, H, W = 2, 3 * ws, 4 * ws
    k = norm_keys(wse, B, H, W, C, dtype)
    sal = focus_map(wse, B, H, W, "f32" if ldsal < 0 else dtype) if kind == "focus" else None
    for k_keep in _keeps(wse * wse):
        check_keybias(run_keybias(sal, ldsal, k, ws, wse, k_keep, dtype), sal, k, ws, wse, k_keep, f"keybias {kind} {dtype}")


@pytest.mark.parametrize("mode", KB_MODES[:3], ids=KB_MODE_IDS[:3])
@pytest.mark.parametrize("win", KB_WINDOWS, ids=[f"ws{w[0]}_wse{w[1]}" for w in KB_WINDOWS])
def test_keybias_tie_block_straddles_the_boundary(win, mode):
    """A 4 x 4 patch of 20.0 next to a 4 x 4 patch of 30.0 inside the interior window's own pixels: tanh = 1 exactly for both, in
    fp32 and in fp64, so 32 keys tie at the top and k_keep = 20 cuts through them: the lowest key indices win."""
    (ws, wse, C), (_, dtype, ldsal) = win, mode
    B, H, W = 2, 3 * ws, 4 * ws
    sal = focus_map(wse + 1, B, H, W, "f32" if ldsal < 0 else dtype)
    sal[:, ws + 2:ws + 6, ws + 1:ws + 5] = 20.0
    sal[:, ws + 2:ws + 6, ws + 5:ws + 9] = 30.0
    assert float(torch.tanh(torch.tensor(20.0, dtype=torch.float64))) == 1.0 and float(torch.tanh(torch.tensor(20.0))) == 1.0
    k = q(rnd("tiek", (B, H, W, C)), dtype)
    ties = check_keybias(run_keybias(sal, ldsal, k, ws, wse, 20, dtype), sal, k, ws, wse, 20, f"tie block {dtype}")
    assert ties >= B, "the planted block does not straddle the boundary of the interior windows"


@pytest.mark.parametrize("mode", KB_MODES[:3], ids=KB_MODE_IDS[:3])
@pytest.mark.parametrize("win", KB_WINDOWS, ids=[f"ws{w[0]}_wse{w[1]}" for w in KB_WINDOWS])
def test_keybias_constant_map_keeps_the_first_keys(win, mode):
    (ws, wse, C), (_, dtype, ldsal) = win, mode
    B, H, W, nk = 2, 3 * ws, 4 * ws, wse * wse
    sal = torch.full((B, H, W), 0.5)
    k = q(rnd("constk", (B, H, W, C)), dtype)
    k_keep = int(0.6 * nk)
    got = run_keybias(sal, ldsal, k, ws, wse, k_keep, dtype)
    assert check_keybias(got, sal, k, ws, wse, k_keep, f"constant map {dtype}") >= 2 * B      # at least the interior windows
    for b in range(B):      # window (1, 1) has no padded key: exactly the first k_keep key indices survive
        assert torch.isfinite(got[b, 1, 1, :nk]).tolist() == [j < k_keep for j in range(nk)]


@pytest.mark.parametrize("mode", KB_MODES[:3], ids=KB_MODE_IDS[:3])
@pytest.mark.parametrize("win", KB_WINDOWS, ids=[f"ws{w[0]}_wse{w[1]}" for w in KB_WINDOWS])
def test_keybias_one_window_frame_padded_keys_outrank_negative_scores(win, mode):
    """A frame of 1 x 1 windows with a negative map: every key outside the image ties at tanh(0) = 0 ABOVE all in-image scores;
    k_keep = 1 and nk / 4 cut through the padded keys (a tie), int(0.6 nk) further down."""
    (ws, wse, C), (_, dtype, ldsal) = win, mode
    B, H, W, nk = 2, ws, ws, wse * wse
    sal = focus_map(wse + 2, B, H, W, "f32" if ldsal < 0 else dtype, lo=-3.0, hi=-0.1)
    k = q(rnd("onek", (B, H, W, C)), dtype)
    assert nk // 4 < nk - ws * ws
    for k_keep, ties in ((1, B), (nk // 4, B), (int(0.6 * nk), None)):
        t = check_keybias(run_keybias(sal, ldsal, k, ws, wse, k_keep, dtype), sal, k, ws, wse, k_keep, f"1x1 windows {dtype}")
        assert ties is None or t == ties


# ------------------------------------------------------------------------------------------------
# hat_ocab_attention_kb — kb is supplied by the test, not taken from the kernel above
# ------------------------------------------------------------------------------------------------
# ws, heads, C, wse -> the kernel hat_ocab_attention_kb reaches (attn_dispatch in csrc/hat_attn.hip; kb never takes the tuned
# ocab_attn_fast_kernel):
#   ws16_d24_wse24   ocab_attn_kernel<T, 36, 12>          (hat_ocab_attention: the same in f32, the tuned kernel in bf16)
#   ws8_d12_wse12    ocab_attn_kernel<T, 9, 9>
#   ws8_d24_wse13    ocab_attn_kernel<T, 11, 11, ODD>
#   ws16_d24_wse25   ocab_attn_kernel<T, 40, 10, ODD>
#   ws16_d30_wse25   bf16: ocab_attn_kernel<bf16, 40, 10, ODD>;  f32: K / V of a key window do not fit the LDS, so
#                    ocab_attn_stream_kernel<float, 40, 10, 4> (hat_ocab_attention streams the same way)
AT_GEOMS = [(16, 6, 144, 24), (8, 2, 24, 12), (8, 2, 48, 13), (16, 6, 144, 25), (16, 6, 180, 25)]
AT_IDS = ["ws16_d24_wse24", "ws8_d12_wse12", "ws8_d24_wse13", "ws16_d24_wse25", "ws16_d30_wse25"]
OVERLAP = {24: 0.5, 12: 0.5, 25: 0.6, 13: 0.7}


def attn_inputs(geom, dtype, zero_table=False):
    ws, heads, C, wse = geom
    B, H, W, d = 2, 3 * ws, 4 * ws, C // heads
    qv = q(rnd("hq", (B, H, W, C)) * d ** -0.5, dtype)
    kv = q(rnd("hkv", (B, H, W, 2 * C)), dtype)
    table = rnd("htab", ((ws + wse - 1) ** 2, heads), std=0.0 if zero_table else 0.5)
    return qv, kv, table


def rand_kb(key, geom, lo=-1.0, hi=1.0):
    """Finite bias, uniform in [lo, hi], a different row per window and per sample; the dead tail is 0."""
    ws, _, _, wse = geom
    nk = wse * wse
    kb = torch.zeros(2, 3, 4, (nk + 15) // 16 * 16)
    kb[..., :nk] = lo + (hi - lo) * torch.rand(2, 3, 4, nk, generator=torch.Generator().manual_seed(key))
    return kb


def run_attention(geom, dtype, qv, kv, table, kb):
    """kb (B, nWy, nWx, nkp) fp32 host tensor -> hat_ocab_attention_kb; None -> hat_ocab_attention.  Padded leading dimensions."""
    ws, heads, C, wse = geom
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W, _ = qv.shape
    M = ws + wse - 1
    rot = (torch.arange(M * M) + (ws - wse + 1 - (ws - 1)) * (M + 1)) % (M * M)      # as test_ocab_attention packs the table
    bias_rot = table[rot].t().contiguous().to(dev)
    ldq, ldkv, ldo = _r8(C), _r8(2 * C), _r8(C) + 8
    out = torch.full((B, H * W, ldo), -77.0, dtype=tdt, device=dev)
    kw = dict(B=B, H=H, W=W, C_=C, heads=heads, ws=ws, wse=wse, ldq=ldq, ldkv=ldkv, ldo=ldo, dtype=dt)
    if kb is None:
        ops.ocab_attention(to_dev(qv, ldq, tdt, dev), to_dev(kv, ldkv, tdt, dev), bias_rot, out, **kw)
    else:
        ops.ocab_attention_kb(to_dev(qv, ldq, tdt, dev), to_dev(kv, ldkv, tdt, dev), bias_rot, kb.float().contiguous().to(dev), out,
                              pad=(wse - ws + 1) // 2, **kw)
    torch.cuda.synchronize()
    assert (out[:, :, C:] == -77.0).all(), "columns past C were written"
    return out[:, :, :C].float().reshape(B, H, W, C).cpu()


def attn_ref(geom, qv, kv, table, kb):
    ws, heads, C, wse = geom
    return ref_attention_kb(qv, kv[..., :C], kv[..., C:], table, O.rpi_oca(ws, OVERLAP[wse]), ws, wse, heads, kb)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geom", AT_GEOMS, ids=AT_IDS)
def test_attention_kb_zero_bias_is_the_plain_attention(geom, dtype):
    """kb = 0: the reference, and hat_ocab_attention on the same inputs within the same bar.  Adding 0.0f changes no logit, so
    wherever both entries run the same instantiation the outputs are bit-identical: every case but ws16_d24_wse24 in bf16, where
    hat_ocab_attention takes the tuned ocab_attn_fast_kernel."""
    qv, kv, table = attn_inputs(geom, dtype)
    kb = torch.zeros_like(rand_kb(0, geom))
    got = run_attention(geom, dtype, qv, kv, table, kb)
    check(got, attn_ref(geom, qv, kv, table, kb), dtype, "attention_kb, zero kb", f32_tol=5e-5)
    plain = run_attention(geom, dtype, qv, kv, table, None)
    check(got, plain, dtype, "attention_kb, zero kb, against hat_ocab_attention", f32_tol=5e-5)
    if not (dtype == "bf16" and geom == AT_GEOMS[0]):
        assert torch.equal(got, plain)


def pruned_kb(key, geom, frac=0.4):
    """A random `frac` of every window's keys pruned (another pattern per window and per sample), random finite bias on the rest."""
    nk = geom[3] ** 2
    kb = rand_kb(key, geom)
    drop = torch.rand(2, 3, 4, nk, generator=torch.Generator().manual_seed(key + 1)) < frac
    kb[..., :nk][drop] = NINF
    assert (~drop).any(-1).all()
    return kb


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("content", ["finite", "pruned40"])
@pytest.mark.parametrize("geom", AT_GEOMS, ids=AT_IDS)
def test_attention_kb_random_bias(geom, content, dtype):
    qv, kv, table = attn_inputs(geom, dtype)
    kb = rand_kb(2, geom) if content == "finite" else pruned_kb(3, geom)
    check(run_attention(geom, dtype, qv, kv, table, kb), attn_ref(geom, qv, kv, table, kb), dtype, f"attention_kb, {content}", f32_tol=5e-5)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geom", AT_GEOMS, ids=AT_IDS)
def test_attention_kb_one_kept_key_copies_its_v_row(geom, dtype):
    """k_keep = 1 and a zero table: the softmax weight of the one kept key is 1 (the others sit 1e4 below it), so every query
    of a window returns that key's V row — zeros when the key lies outside the image — to the storage type's rounding.  A window
    offset, a key index or a kb row stride that is off by one picks another pixel."""
    ws, heads, C, wse = geom
    qv, kv, table = attn_inputs(geom, dtype, zero_table=True)
    B, H, W, nk, pad, d = 2, 3 * ws, 4 * ws, wse * wse, (wse - ws + 1) // 2, C // heads
    kept = torch.randint(0, nk, (B, 3, 4), generator=torch.Generator().manual_seed(4))
    kept[0, 0, 0], kept[1, 2, 3], kept[0, 1, 1], kept[1, 1, 2] = 0, nk - 1, nk - 1, 0      # padded corners; first / last key
    kb = torch.zeros(B, 3, 4, (nk + 15) // 16 * 16)
    kb[..., :nk] = NINF
    kb.scatter_(-1, kept[..., None], 0.25)
    want = torch.zeros(B, H, W, C)
    for b in range(B):
        for wy in range(3):
            for wx in range(4):
                key = int(kept[b, wy, wx])
                y, x = wy * ws - pad + key // wse, wx * ws - pad + key % wse
                if 0 <= y < H and 0 <= x < W:
                    want[b, wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws] = kv[b, y, x, C:]
    got = run_attention(geom, dtype, qv, kv, table, kb)
    eps = torch.finfo(torch.bfloat16 if dtype == "bf16" else torch.float32).eps
    err = (got.double() - want.double()).abs()
    assert (err <= eps * want.double().abs()).all(), f"max-abs {float(err.max()):.3e} at {(err == err.max()).nonzero()[0].tolist()}"
    check(got, attn_ref(geom, qv, kv, table, kb), dtype, "attention_kb, one kept key", f32_tol=5e-5)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geom", AT_GEOMS, ids=AT_IDS)
def test_attention_kb_pruned_keys_contribute_nothing(geom, dtype):
    """40 % of the pixels are pruned in every window that sees them; their K rows are scaled x40 (unpruned, their logits would
    dominate) and their V rows are 1e3 (any weight at all shows)."""
    ws, heads, C, wse = geom
    qv, kv, table = attn_inputs(geom, dtype)
    B, H, W, nk, pad = 2, 3 * ws, 4 * ws, wse * wse, (wse - ws + 1) // 2
    dead = torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) < 0.4
    kv[..., :C][dead] *= 40.0
    kv[..., C:][dead] = 1.0e3
    kv = q(kv, dtype)
    kb = rand_kb(6, geom)
    kb[..., :nk][key_windows(dead, ws, wse, pad)[0]] = NINF
    assert torch.isfinite(kb[..., :nk]).any(-1).all()
    ref = attn_ref(geom, qv, kv, table, kb)
    assert float(ref.abs().max()) < 10.0
    check(run_attention(geom, dtype, qv, kv, table, kb), ref, dtype, "attention_kb, loud pruned keys", f32_tol=5e-5)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geom", AT_GEOMS, ids=AT_IDS)
def test_attention_kb_pruned_logit_is_replaced_not_shifted(geom, dtype):
    """A pruned key's logit is -1e4 whatever q.k is.  That only shows when the kept keys sit at -1e4 too: here the kept keys are
    the zero-padded ones and 10 % of the pixels, whose K rows are zeroed (logit exactly 0) and whose kb is -1e4; with a zero table
    every logit of a window is then exactly -1e4 and the output is the plain mean of the window's V rows.  -1e4 + q.k for the
    pruned keys would weight them by exp(q.k) instead."""
    ws, heads, C, wse = geom
    qv, kv, table = attn_inputs(geom, dtype, zero_table=True)
    B, H, W, nk, pad = 2, 3 * ws, 4 * ws, wse * wse, (wse - ws + 1) // 2
    quiet = torch.rand(B, H, W, generator=torch.Generator().manual_seed(7)) < 0.1
    kv[..., :C][quiet] = 0.0
    pruned = key_windows(~quiet, ws, wse, pad)[0]                # (padded keys read 0 = False: kept)
    assert (~pruned).any(-1).all() and pruned.any(-1).all()
    kb = torch.zeros(B, 3, 4, (nk + 15) // 16 * 16)
    kb[..., :nk] = torch.where(pruned, torch.tensor(NINF), torch.tensor(-1.0e4))
    ref = attn_ref(geom, qv, kv, table, kb)
    mean_v = key_windows(kv[..., C:].double(), ws, wse, pad)[0].mean(3)          # (B, nWy, nWx, C)
    assert float((ref.reshape(B, 3, ws, 4, ws, C) - mean_v[:, :, None, :, None, :]).abs().max()) <= 1e-12
    check(run_attention(geom, dtype, qv, kv, table, kb), ref, dtype, "attention_kb, every logit at -1e4", f32_tol=5e-5)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geom", AT_GEOMS[2:], ids=AT_IDS[2:])
def test_attention_kb_ignores_the_dead_tail_of_odd_windows(geom, dtype):
    """Odd key windows are padded to whole 16-key tiles; the header says the attention kernel ignores kb there.  1e30 and -inf
    in [nk, nkp) leave the result of the 40 %-pruned case unchanged, bit for bit."""
    nk = geom[3] ** 2
    qv, kv, table = attn_inputs(geom, dtype)
    kb = pruned_kb(3, geom)
    assert kb.shape[-1] > nk
    clean = run_attention(geom, dtype, qv, kv, table, kb)
    kb[..., nk:] = 1.0e30
    kb[:, ::2, 1::2, nk:] = NINF
    kb[1, 1, 1, nk:] = -1.0e30
    assert torch.equal(run_attention(geom, dtype, qv, kv, table, kb), clean)
    check(clean, attn_ref(geom, qv, kv, table, kb), dtype, "attention_kb, garbage in the dead tail", f32_tol=5e-5)


# ------------------------------------------------------------------------------------------------
# hat_sgfn_gate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded_ld"])
@pytest.mark.parametrize("geom", [(2, 19, 23), (1, 3, 5), (1, 1, 7), (1, 40, 64)], ids=["B2_19x23", "3x5", "1x7", "40x64"])
@pytest.mark.parametrize("half", [36, 144, 360])
def test_sgfn_gate(half, geom, padded, dtype):
    """half 36: the tiny goldens; 144: hatx_sgfn_c144; 360: the live config's 720-wide hidden layer."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    B, H, W = geom
    u = q(rnd("sgu", (B, H, W, 2 * half)), dtype)
    wd, bd = rnd("sgw", (half, 1, 3, 3), std=1 / 3), rnd("sgb", (half,), std=0.1)
    ref = ref_sgfn_gate(u, wd, bd, half)
    ldu = ldo = (_r8(2 * half) + 8) if padded else 2 * half
    ud = torch.full((B, H * W, ldu), 55.0, dtype=tdt, device=dev)                # (pad columns of u are not zero either)
    ud[:, :, :2 * half] = u.reshape(B, H * W, 2 * half).to(dev).to(tdt)
    wdev, bdev = wd.reshape(half, 9).t().contiguous().to(dev), bd.to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((B, H * W, ldo), -77.0, dtype=tdt, device=dev)
        ops.sgfn_gate(ud, wdev, bdev, out, B=B, H=H, W=W, half=half, ldu=ldu, ldo=ldo, dtype=dt)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    out = outs[0]
    check(out[:, :, :half].float().reshape(B, H, W, half), ref[..., :half], dtype, "sgfn gate, gated half")
    assert torch.equal(out[:, :, half:2 * half], ud[:, :, half:2 * half].cpu()), "the pass-through half is not a copy"
    assert (out[:, :, 2 * half:] == -77.0).all(), "columns past 2 * half were written"
    assert torch.equal(outs[1], out), "a second call differs"


# ------------------------------------------------------------------------------------------------
# hat_add_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("broadcast", [False, True], ids=["c_per_sample", "c_broadcast"])
@pytest.mark.parametrize("n", [4, 1028, 4096 * 256 * 4 + 12], ids=["n4", "n1028", "past_one_grid_sweep"])
@pytest.mark.parametrize("B", [1, 3])
def test_add_f32(B, n, broadcast, inplace):
    """out = a + c exactly; c_bstride = 0 broadcasts one c over the batch; the 16 floats after the last valid element stay."""
    dev, ops = _dev(), _ops()
    g = torch.Generator().manual_seed(B * 1000 + n % 1000)
    a = torch.randn(B, n, generator=g)
    c = torch.randn(1 if broadcast else B, n, generator=g)
    want = a + c
    tail = 16
    ad = torch.full((B * n + tail,), -77.0, device=dev)
    ad[:B * n] = a.reshape(-1).to(dev)
    od = ad if inplace else torch.full((B * n + tail,), -77.0, device=dev)
    ops.add_f32(ad, c.reshape(-1).contiguous().to(dev), od, B=B, n=n, c_bstride=0 if broadcast else n)
    torch.cuda.synchronize()
    assert torch.equal(od[:B * n].cpu().reshape(B, n), want)
    assert (od[B * n:] == -77.0).all(), "elements past the end were written"
    if not inplace:
        assert torch.equal(ad[:B * n].cpu().reshape(B, n), a), "the input was modified"
