"""Host-side checks of tests/wmsa_cases.py: the index-arithmetic restatement of hat_window_attention is the oracle's (S)W-MSA, every
deliberately wrong variant of it (SLIPS) leaves the bf16 bars of helpers.check by a factor of two on at least one case family, and
the mask cases put the masked key where they say.  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

import wmsa_cases as WC
from helpers import wmsa_sd
from oracle import hat_oracle as O
from super_resolution_amd import synth

# one window, one window row, one window column, 2 x 3 windows (in windows; the frame is ws times that)
FRAMES = [(1, 1), (1, 3), (3, 1), (2, 3)]


@pytest.mark.parametrize("ws,heads", [(16, 2), (8, 6)])
def test_restatement_is_the_oracle(ws, heads):
    """wmsa_core on q, k, v = F.linear of a seeded wmsa_sd, followed by the projection, against O.window_msa, in fp64."""
    C = 48
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in wmsa_sd(C, heads, ws).items()}
    sd["relative_position_bias_table"] = sd["relative_position_bias_table"] * 4.0     # (std 2: bias and mask both matter)
    for ny, nx in FRAMES:
        x = synth.normal(5, f"wmr{ws}.{ny}x{nx}", (2, ny * ws, nx * ws, C)).double()
        qkv = F.linear(x, sd["qkv.weight"], sd["qkv.bias"])
        qv, k, v = qkv[..., :C] * (C // heads) ** -0.5, qkv[..., C:2 * C], qkv[..., 2 * C:]
        for shift in WC.SHIFTS[ws]:
            got = F.linear(WC.wmsa_core(qv, k, v, sd["relative_position_bias_table"], ws, heads, shift), sd["proj.weight"], sd["proj.bias"])
            ref = O.window_msa(x, {"a." + key: t for key, t in sd.items()}, "a", ws, heads, shift)
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            assert err <= 1e-12, f"ws {ws} frame {ny}x{nx} windows shift {shift}: {err:.3e}"


def test_index_is_the_modules():
    """The table lookup wmsa_core restates is the registered relative_position_index, and bias_flip is what the module packs."""
    from super_resolution_amd.archs.window_msa import relative_position_index
    for ws in (8, 16):
        assert torch.equal(relative_position_index(ws), O.rpi_sa(ws))
        c = WC.random_case(48, 2, ws, WC.MAIN[ws])
        n, M = ws * ws, 2 * ws - 1
        i = torch.arange(n)
        kq = ((i // ws)[None, :] - (i // ws)[:, None] + ws - 1) * M + ((i % ws)[None, :] - (i % ws)[:, None] + ws - 1)   # key - query
        assert torch.equal(c.bias_flip[:, kq.reshape(-1)], c.table[O.rpi_sa(ws).reshape(-1)].t())


# ------------------------------------------------------------------------------------------------
# every slip is visible
# ------------------------------------------------------------------------------------------------
def _families(ws):
    """family -> the cases of it that test_gpu_wmsa.py launches at this window size (operands rounded to bf16: the wider bars)."""
    kw = dict(dtype="bf16")
    return {
        "random": [WC.random_case(48, 2, ws, WC.MAIN[ws], s, **kw) for s in WC.SHIFTS[ws]],
        "mask": [WC.mask_case(ws, s, over, **kw) for s in WC.SHIFTS[ws] if s for over in (True, False)],
        "selector": [WC.selector_case(ws, s, dy, dx, **kw) for s in WC.SHIFTS[ws] for dy, dx in WC.selector_offsets(ws)],
        "spike": [WC.spike_case(ws, s, where, **kw) for s in (0, 4) for where in WC.SPIKES],
    }


def _separation(case, slip):
    """How far the slip moves the case, in units of TWICE the bf16 bars of helpers.check (rel 1.2e-2, max-abs 6e-2 * scale): >= 1 is
    beyond both doubled bars' reach, i.e. caught."""
    ref, bad = case.ref, case.core(slip)
    if not torch.isfinite(bad).all():
        return float("inf")
    scale = max(float(ref.abs().max()), 1.0)
    return max(float((bad - ref).norm() / ref.norm()) / 2.4e-2, float((bad - ref).abs().max()) / (12e-2 * scale))


@functools.lru_cache(maxsize=None)
def _slip_table(ws):
    fam = _families(ws)
    return {slip: {name: max(_separation(c, slip) for c in cases) for name, cases in fam.items()} for slip in WC.SLIPS}


@pytest.mark.parametrize("ws", [16, 8])
def test_every_slip_is_visible(ws):
    table = _slip_table(ws)
    print(f"\nws {ws}: separation of each slip from the restatement per case family, in units of twice the bf16 bars (>= 1: caught)")
    for slip, row in table.items():
        caught = [name for name, s in row.items() if s >= 1.0]
        print(f"  {slip:20s} " + "  ".join(f"{name} {s:9.3g}" for name, s in row.items()) + "   caught by: " + (", ".join(caught) or ("NOTHING" if max(row.values()) else "(not a slip at this ws: identical)")))
    for slip, row in table.items():
        if slip == "bands_swapped" and all(s in (0, ws - s) for s in WC.SHIFTS[ws]):
            # ws 8 admits the shifts 0 and 4 = ws - 4 only: swapping `shift` and `ws - shift` is the same function there, not a slip
            # that goes unseen (ws 16 has shifts 4 and 12, where it is caught)
            assert ws == 8 and max(row.values()) == 0.0, (ws, row)
            continue
        assert max(row.values()) >= 1.0, f"ws {ws}: no case family separates {slip}: {row}"
    for slip in ("mask_replaces", "mask_minus_inf", "mask_adds_twice"):           # by construction
        assert table[slip]["mask"] >= 1.0, (slip, table[slip])
    for slip in ("bias_not_flipped", "bias_transposed", "roll_reversed", "no_wrap"):
        assert table[slip]["selector"] >= 1.0, (slip, table[slip])


@pytest.mark.parametrize("ws", [16, 8])
def test_mask_pairs_take_all_or_nothing(ws):
    """over=True: the masked key of each pair holds > 0.999 of its query's softmax; over=False: < 1e-12 — in fp64, on every head and
    sample.  Both are what ADDING -100 once gives: 130 - 100 = 30 against zeros, 60 - 100 = -40."""
    for shift in WC.SHIFTS[ws]:
        if not shift:
            continue
        for over in (True, False):
            c = WC.mask_case(ws, shift, over)
            p = c.core(probs=True)[1]
            assert len(c.pairs) == 3
            for wy, wx, qi, kj in c.pairs:
                w = p[:, wy, wx, :, qi, kj]
                assert bool((w > 0.999).all() if over else (w < 1e-12).all()), (ws, shift, over, (wy, wx, qi, kj), w)


@pytest.mark.parametrize("ws", [16, 8])
def test_selector_returns_the_selected_key(ws):
    """Channels 0 / 1 of the reference name the pixel that was read: for a query whose offset key lies in its window and band, the
    key's own pixel; and on every frame some query selects and (with a shift) some query is refused by the mask."""
    H, W, B = WC.MAIN[ws]
    for shift in WC.SHIFTS[ws]:
        for dy, dx in WC.selector_offsets(ws):
            c = WC.selector_case(ws, shift, dy, dx)
            band = lambda t, size: int(t >= size - ws) + int(t >= size - shift)
            hit = masked = 0
            for fy in range(H):
                for fx in range(W):
                    ky, kx = fy + dy, fx + dx
                    if not (fy // ws == ky // ws and fx // ws == kx // ws and 0 <= ky and 0 <= kx):
                        continue
                    if (band(fy, H), band(fx, W)) != (band(ky, H), band(kx, W)):
                        masked += 1
                        continue
                    hit += 1
                    got = c.ref[:, (fy + shift) % H, (fx + shift) % W, :2]
                    want = torch.tensor([((ky + shift) % H) / ws, ((kx + shift) % W) / ws], dtype=torch.float64)
                    assert float((got - want).abs().max()) <= 1e-9, (ws, shift, (dy, dx), (fy, fx), got)
            assert hit > 0 and (masked > 0) == (shift > 0 and (dy, dx) != (0, 0)), (ws, shift, (dy, dx), hit, masked)


def test_case_matrix_is_the_issues():
    """The full geometry x shift product for fast24, fast30 and f32 d24; every other row on the main frame at shifts 0, 4 and the
    largest; nothing larger than 64 x 48 x 180."""
    m = WC.core_matrix()
    full = [r for r in WC.CASES if r[4]]
    assert [(r[0], r[2] // r[3]) for r in full] == [("f32", 24), ("bf16", 24), ("bf16", 30)]
    assert len(m) == 3 * 6 * 4 + 9 * 3 + 6 * 2
    assert {(r[0], r[1], r[2] // r[3]) for r in WC.CASES} >= {("f32", 16, d) for d in (24, 30, 32, 16, 10, 6, 2)} | {("bf16", 16, d) for d in (24, 30, 32, 16, 10)}
    for row, (H, W, B), s in m:
        assert H * W <= 64 * 48 and row[2] <= 180 and s in WC.SHIFTS[row[1]]
    assert {H // 16 * (W // 16) * B for H, W, B in WC.GEOMS[16]} == {1, 3, 12, 8, 9}
