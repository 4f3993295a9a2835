"""What tests/test_gpu_escreal_edges.py and the MLP-term bar of tests/test_gpu_esclte.py rest on, without a GPU: dysample_from_rows
(the restatement of hat_dysample on its own rows) against the head restated from the feature map, banded against unbanded; the fp64
bilinear base image against F.grid_sample; the MLP-term quantity with one 16-channel group of the last hidden layer dropped, which
has to fall outside the bar; and the arithmetic of every need_trips call of the GPU file."""
import pytest
import torch
import torch.nn.functional as F

import esclte_ref as L
import escreal_ref as R
import test_gpu_escreal_edges as G
from helpers import max_abs, need_trips, rnd

BF16_REL = 1.2e-2   # helpers.check's bf16 bar on the relative L2 error


def _dys_rows(s, B=2, H=9, W=13):
    from super_resolution_amd import packing
    sd = R.d64(R.load_case({2: "e", 3: "d", 4: "c"}[s])[1])
    wd, bd = packing.dysample_fold(sd["to_img.offset.weight"], sd["to_img.offset.bias"], sd["to_img.scope.weight"], sd["to_img.end_conv.weight"])
    feat = rnd(f"dysref{s}", (B, 64, H, W)).double()
    rows = torch.full((B, H * W, wd.shape[0] + 4), float("nan"), dtype=torch.float64)
    rows[:, :, :wd.shape[0]] = F.conv2d(feat, wd[:, :, None, None], bd).reshape(B, wd.shape[0], H * W).transpose(1, 2)
    return sd, feat, rows


@pytest.mark.parametrize("s", [2, 3, 4])
def test_dysample_from_rows_is_the_head(s):
    B, H, W = 2, 9, 13
    sd, feat, rows = _dys_rows(s, B, H, W)
    px, py = R.dys_positions(feat[:1], sd, s)
    assert (px < 0).any() and (px > W - 1).any() and (py < 0).any() and (py > H - 1).any()      # the clamp is live on every side
    got = R.dysample_from_rows(rows, sd["to_img.init_pos"].reshape(-1), sd["to_img.end_conv.bias"], H, W, s)
    assert tuple(got.shape) == (B, 3, s * H, s * W) and bool(torch.isfinite(got).all())
    for b in range(B):
        assert max_abs(got[b:b + 1], R.head_dysample(feat[b:b + 1], sd, s)) <= 1e-12
        assert max_abs(got[b:b + 1], R.head_dysample(feat[b:b + 1], sd, s, project_first=True)) <= 1e-12
    assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("band", [1, 2, 4, 9, 50])
def test_dysample_from_rows_banded_is_unbanded(band):
    s, H, W = 4, 9, 13
    sd, _, rows = _dys_rows(s, 2, H, W)
    ip, bias = sd["to_img.init_pos"].reshape(-1), sd["to_img.end_conv.bias"]
    assert torch.equal(R.dysample_from_rows(rows, ip, bias, H, W, s, band=band), R.dysample_from_rows(rows, ip, bias, H, W, s))


@pytest.mark.parametrize("hw", [(5, 7), (1, 3), (1, 1), (3, 1)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_bilinear_base_is_grid_sample(hw):
    H, W = hw
    inp = rnd(f"base{H}x{W}", (1, 3, H, W), std=0.5).double()
    for coord in (L.scatter_queries(f"base.q{H}x{W}", 143, HW=hw)[0], L.make_coord((11, 13)), L.make_coord((H, W)), L.make_coord((3, 4))):
        c = coord[None].double()
        want = F.grid_sample(inp, c.flip(-1).unsqueeze(1), mode="bilinear", padding_mode="border", align_corners=False)[:, :, 0, :].permute(0, 2, 1)
        assert max_abs(L.bilinear_base(inp, c), want) <= 1e-12


def _mlp_terms(H, W, Q):
    """-> (the MLP term of the fp64 head with bf16 MFMA weights, fn: state dict -> MLP term, fn: the fp32 emulation's MLP term)."""
    from test_gpu_esclte import head_case, head_ref
    coef, freq, inp = head_case(H, W)
    coord, cell, _ = head_ref(H, W, ("scatter", Q))
    sd = L.mfma_weights_as_bf16(L.head_state_dict())
    base = L.bilinear_base(inp.double(), coord[None].double())[0]
    run = lambda sd_: L.head(L.d64(sd_), coef.double(), freq.double(), inp.double(), coord[None].double(), cell[None].double())[0] - base
    emu = lambda: L.head(sd, coef, freq, inp, coord[None], cell[None], act_round=L.bf16_round)[0].double() - base
    return run(sd), run, sd, emu


def test_a_dropped_hidden_group_moves_the_mlp_term_beyond_the_bar():
    """The quantity mlp_bar judges — the relative L2 error of (y - base) against the fp64 head with bf16 MFMA weights — with one
    16-channel group of the last hidden layer dropped, for every group: each lies far outside the bf16 bar, while the torch fp32
    emulation that rounds the basis and the first two hidden layers to bf16 (the kernel's three roundings) lies inside it."""
    ref, run, sd, emu = _mlp_terms(5, 7, L.N_SCATTER)
    rels = [float((run(L.without_hidden_group(sd, g)) - ref).norm() / ref.norm()) for g in range(16)]
    e = float((emu() - ref).norm() / ref.norm())
    print(f"MLP term, 143 queries on 5x7: one group dropped -> rel {min(rels):.3e} .. {max(rels):.3e}; bf16 emulation rel {e:.3e}; bar {BF16_REL}")
    assert min(rels) > 4 * BF16_REL, rels
    assert e <= BF16_REL, e
    # the image bar alone would not notice: 40 dB on y * 0.5 + 0.5 is an RMS error of 1e-2 in image units
    assert L.psnr(ref * 0.5 + 0.5, ref * 0.5 + 0.5 + 1e-3) > 40.0


MT_CASES = ([("hat_unshuffle_pad", G.unshuf_units(f, B, Hb, Wb), B, G.UNSHUF_TRIP_VALUES) for f, cs in G.UNSHUF_MT.items() for B, Hb, Wb, _ in cs]
            + [("hat_shuffle_planes", G.shuffle_units(s, B, H, W), B, G.SHUFP_TRIP_OUTPUTS) for s, cs in G.SHUFP_MT.items() for B, H, W in cs]
            + [("hat_escfp_shuffle_bicubic", G.shuffle_units(s, *c), c[0], G.BICUBIC_TRIP_OUTPUTS) for s, c in G.BICUBIC_MT.items()]
            + [("hat_dysample", G.dys_units(*G.DYS_MT), G.DYS_MT[0], G.DYS_TRIP_PIXELS)])


@pytest.mark.parametrize("case", MT_CASES, ids=lambda c: f"{c[0]}_{c[1]}")
def test_multitrip_shapes_take_three_ragged_trips(case):
    what, units, B, cap = case
    hi, lo = need_trips(units, cap, 3, what)
    assert hi >= 3 and lo == hi - 1 and units % cap != 0
    if B == 2:
        assert (units // 2) % cap != 0 and cap < units // 2 < 2 * cap, "sample 1 does not start inside the second trip"


def test_multitrip_shapes_cover_what_the_gpu_file_runs():
    assert set(G.UNSHUF_MT) == {2, 4} and set(G.SHUFP_MT) == {2, 4} and set(G.BICUBIC_MT) == {2, 3, 4} and G.DYS_MT[3] == 4
    assert any(c[0] == 2 for c in G.UNSHUF_MT[2]) and any(c[0] == 2 for c in G.SHUFP_MT[2]) and G.DYS_MT[0] == 2
    for cs in G.UNSHUF_MT.values():
        assert all(ph >= 1 and pw >= 1 for _, _, _, (ph, pw) in cs), "a reflect pad of the unshuffle is dead"
    assert G.UNSHUF_TRIP_VALUES == G.SHUFP_TRIP_OUTPUTS == G.BICUBIC_TRIP_OUTPUTS == 8192 * 256 and G.DYS_TRIP_PIXELS == 16384 * 256
