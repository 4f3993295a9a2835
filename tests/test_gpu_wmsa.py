"""hat_window_attention called directly, through ops.window_attention, on operands the tests control (tests/wmsa_cases.py), against
the fp64 restatement of the same operation on the same rounded operands.  Until now the entry was reached only behind a seeded qkv
projection (test_window_msa_* in test_gpu_ops.py).

The launches are reported under one name whichever kernel ran, so the tests pick their kernel through the dispatch conditions of
hat_window_attention: bf16, ws 16, head size 24 with ldq % 8 == ldkv % 8 == ldo % 4 == 0, q / kv on 16 and out on 8
bytes -> ocab_attn_fast_kernel<24, 16, true>; bf16, ws 16, head size 30 with even strides -> <30, 16, true>; anything else the
generic ocab_attn_kernel<T, ws^2 / 16, chunk, true>.

Bars: helpers.check as it stands — bf16 rel 1.2e-2 / max-abs 6e-2 * scale; f32 max-abs 5e-5 * scale as test_ocab_attention, 1e-4
for the logit spikes as test_ocab_attention_softmax_spike.  test_wmsa_ref_cpu.py shows that each slip of wmsa_cases.SLIPS moves
one of these case families by twice the bf16 bars."""
import pytest
import torch

import wmsa_cases as WC
from helpers import _r8, check, fill_rows, pads_keep

pytestmark = pytest.mark.gpu

F32_TOL, SPIKE_TOL = 5e-5, 1e-4
FAM_ID = lambda f: f"{f[0]}-ws{f[1]}-C{f[2]}"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    from super_resolution_amd import ops
    return ops


def _run(c, *, ld3=None, split=None, ldo=None, q_lead=0, fill=0.0, out_fill=0.0):
    """One launch on the case's operands -> the raw (B, H*W, ldo) output rows.  Default layout: the module's — one qkv map of row stride
    round8(3C) with q = base, kv = base + C, zero pad channels, ldo = round8(C).  ld3: another stride for that map.  split = (ldq,
    ldkv): q and k|v in buffers of their own; q_lead: q starts that many elements into its buffer.  fill: what the pad channels of
    q / kv hold; out_fill: what out holds before the launch."""
    dev, ops = _dev(), _ops()
    dt = ops.DTYPE_CODE[c.dtype]
    tdt = ops.TORCH_DTYPE[dt]
    H, W, B = c.geom
    C = c.C
    ldo = ldo or _r8(C)
    out = torch.full((B, H * W, ldo), out_fill, dtype=tdt, device=dev)
    if split is None:
        ldq = ldkv = ld3 or _r8(3 * C)
        qb = fill_rows(torch.cat([c.q, c.k, c.v], -1), ldq, tdt, dev, fill)
        kvb = qb.view(-1)[C:]
    else:
        ldq, ldkv = split
        rows = fill_rows(c.q, ldq, tdt, dev, fill)
        buf = torch.zeros(q_lead + rows.numel(), dtype=tdt, device=dev)
        buf[q_lead:] = rows.view(-1)
        qb = buf[q_lead:]
        kvb = fill_rows(torch.cat([c.k, c.v], -1), ldkv, tdt, dev, fill)
    ops.window_attention(qb, kvb, c.bias_flip.to(dev), out, B=B, H=H, W=W, C_=C, heads=c.heads, ws=c.ws, shift=c.shift, ldq=ldq,
                         ldkv=ldkv, ldo=ldo, dtype=dt)
    torch.cuda.synchronize()
    return out


def _live(out, c):
    H, W, B = c.geom
    return out[:, :, :c.C].float().reshape(B, H, W, c.C)


def _judge(out, c, f32_tol=F32_TOL, what=""):
    check(_live(out, c), c.ref, c.dtype, c.name + what, f32_tol=f32_tol)


@pytest.mark.parametrize("row,geom,shift", WC.core_matrix(),
                         ids=[f"{WC.ROW_ID(r)}-{g[0]}x{g[1]}x{g[2]}-shift{s}" for r, g, s in WC.core_matrix()])
def test_core_matches_fp64(row, geom, shift):
    """Every kernel and head size, on Gaussian operands under a bias table of std 2: one-window, one-row and one-column frames, 8, 9
    and 12 windows, every legal shift (at shift 4 the first key chunk of the last window row's query rows >= 12 is masked as a whole)."""
    dtype, ws, C, heads, _ = row
    c = WC.random_case(C, heads, ws, geom, shift, dtype)
    _judge(_run(c), c)


@pytest.mark.parametrize("over", [True, False], ids=["over", "under"])
@pytest.mark.parametrize("row", WC.CASES, ids=WC.ROW_ID)
def test_mask_is_added_not_substituted(row, over):
    """-100 is ADDED, once: a pair with q.k = 130 across bands keeps logit 30 and takes the whole softmax (a kernel that substitutes
    -100 or -inf, or adds -200 in the corner window, gives the band's mean instead); one with q.k = 60 keeps -40 and takes none."""
    dtype, ws, C, heads, _ = row
    for shift in WC.SHIFTS[ws][1:]:
        c = WC.mask_case(ws, shift, over, C, heads, None, dtype)
        _judge(_run(c), c)


@pytest.mark.parametrize("offset", range(4))
@pytest.mark.parametrize("fam", [f for f in WC.FAMILIES if f != ("bf16", 16, 64, 2)], ids=FAM_ID)
def test_selector_bias_orientation(fam, offset):
    """q = 0 and one table entry at +40: each query returns the v row of the key at that offset from it — which names its pixel in
    channels 0 / 1 — where window and band allow, else its band's mean.  Orientation of the table (flip, dy / dx), the direction of
    the cyclic shift and the wrap at the frame edge all move which pixel that is."""
    dtype, ws, C, heads = fam
    dy, dx = WC.selector_offsets(ws)[offset]      # (0, 0), (ws-1, ws-1), (-(ws-1), ws-1), (3, -5)
    for shift in WC.SHIFTS[ws]:
        c = WC.selector_case(ws, shift, dy, dx, C, heads, None, dtype)
        _judge(_run(c), c)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("where", WC.SPIKES)
@pytest.mark.parametrize("fam", [f for f in WC.FAMILIES if f[1] == 16], ids=FAM_ID)
def test_softmax_rescale_in_self_kernels(fam, where, shift):
    """One key of every window with k times 40: in the last chunk (everything before it is rescaled), in the first (every later chunk
    underflows against it), and in the other band of the last window row (the spike competes through the -100)."""
    dtype, ws, C, heads = fam
    c = WC.spike_case(ws, shift, where, C, heads, None, dtype)
    _judge(_run(c), c, f32_tol=SPIKE_TOL)


@pytest.mark.parametrize("variant", ["aligned", "ldo_146", "q_one_element_in", "ldq_3C_plus_2"])
def test_fast_preconditions_fall_back_and_agree(variant):
    """C = 144 in bf16: the aligned call takes the fast kernel; an out stride that is no multiple of 4, a q pointer 2 bytes off a
    16-byte boundary and a row stride that is no multiple of 8 each fail one of its preconditions and must take the generic bf16
    kernel at ws 16 (which nothing else reaches with head size 24) — every one to the same fp64 reference at the bf16 bars."""
    C = 144
    c = WC.random_case(C, 6, 16, WC.MAIN[16], 8, "bf16")
    kw = {"aligned": dict(), "ldo_146": dict(ldo=146), "q_one_element_in": dict(split=(C, 2 * C), q_lead=1),
          "ldq_3C_plus_2": dict(ld3=3 * C + 2)}[variant]
    _judge(_run(c, **kw), c, what=" " + variant)


def test_fast30_pointer_two_bytes_off_falls_back_and_agrees():
    """C = 180 in bf16 with q one element into its buffer: the head-size-30 kernel moves 4 bytes at a time, so the call goes to the
    generic kernel (bf16, ws 16, head size 30: reached by nothing else)."""
    c = WC.random_case(180, 6, 16, WC.MAIN[16], 8, "bf16")
    _judge(_run(c, split=(180, 360), q_lead=1), c, what=" q one element in")


@pytest.mark.parametrize("fam", WC.FAMILIES, ids=FAM_ID)
def test_layout(fam):
    """q and k|v in buffers of their own with three different strides, NaN in every pad channel of q / kv and 7.0 all over out: the
    live columns match, the pad columns of out are untouched, nothing is non-finite; and the same operands as one packed qkv map
    (kv = base + C) give the same bits."""
    dtype, ws, C, heads = fam
    c = WC.random_case(C, heads, ws, WC.MAIN[ws], 4, dtype)
    out = _run(c, split=(C + 8, 2 * C + 16), ldo=C + 8, fill=float("nan"), out_fill=7.0)
    _judge(out, c, what=" split buffers")
    pads_keep(out, C, 7.0, c.name)
    packed = _run(c, ld3=3 * C, ldo=C + 8, out_fill=7.0)
    pads_keep(packed, C, 7.0, c.name + " packed")
    assert torch.equal(out[..., :C], packed[..., :C]), c.name + ": split and packed operands differ"


@pytest.mark.parametrize("fam", WC.FAMILIES, ids=FAM_ID)
def test_each_sample_and_window_is_independent(fam):
    """B = 2 with different samples equals two B = 1 calls bit for bit (the sample / window index arithmetic; with the fast kernel the
    windows are also dealt to the workgroups differently)."""
    dtype, ws, C, heads = fam
    c = WC.random_case(C, heads, ws, WC.MAIN[ws], 4, dtype)
    H, W, B = c.geom
    assert B == 2 and not torch.equal(c.q[0], c.q[1])
    both = _run(c)
    for b in range(B):
        one = WC.Case(f"{c.name} sample {b}", dtype, ws, heads, c.shift, (H, W, 1), c.q[b:b + 1], c.k[b:b + 1], c.v[b:b + 1], c.table)
        assert torch.equal(_run(one)[0], both[b]), one.name
