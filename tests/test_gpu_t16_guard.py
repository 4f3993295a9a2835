"""The FP16-range guard of the residual stream.

Kernel level: hat_hab_tail3_guarded, hat_conv_guarded and hat_linear_guarded store what their unguarded entries store, bit for
bit, and raise one word to the bit pattern of the largest magnitude their FP16 stores clipped.  The reference for that word is
the UNGUARDED entry's fp32-row launch on the same inputs: the FP16-row launch is the same arithmetic with another store
(tests/test_gpu_fp16_stream.py, test_gpu_ops.test_hab_tail3_fp16_residual_rows pin that), so its fp32 rows are the values the
guarded launch converts.  Engine level: a model whose stream leaves the FP16 range is detected and runs on the fp32 stream."""
import struct
import warnings

import pytest
import torch
import torch.nn.functional as F

from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

C, LIM = 144, 65504.0
GEOMS = {"tail": [(2, 24, 40), (1, 19, 27)], "conv": [(2, 24, 40), (1, 19, 27)], "proj": [(2, 16, 40), (1, 19, 27)]}
CASES = [(k, g) for k in ("tail", "conv", "proj") for g in GEOMS[k]]
IDS = [f"{k}_B{g[0]}_{g[1]}x{g[2]}" for k, g in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(key, shape, std=1.0):
    return synth.normal(23, key, shape, std=std)


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", abs(float(v))))[0]


def same(a, b):
    """bit equality (NaN == NaN of the same pattern)"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


class Driver:
    """One of the three FP16-row producers on fixed operands.  run(t, in_half, out_half, sat, bump) launches it on the residual
    stream t (B, N, C) fp32 master (handed over as FP16 rows with in_half) and returns its outputs on the host: (rows, LayerNorm
    rows, pool partials, compact copy).  bump = (channel, value) is added to the launch's fp32 bias for that launch.  pad: the
    stream buffer has that many more pixels behind the last one (never read: the kernels clamp their addresses)."""

    def __init__(self, kind, geom, dev):
        from super_resolution_amd import ops
        self.ops, self.kind, self.dev = ops, kind, dev
        self.B, self.H, self.W = B, H, W = geom
        self.N = N = H * W
        dt, tdt = ops.HAT_BF16, torch.bfloat16
        self.base = (rnd(kind + "t", (B, N, C), std=1.5) + 0.3).half().float()
        self.lg, self.lb = (1 + rnd(kind + "lg", (C,), std=0.1)).to(dev), rnd(kind + "lb", (C,), std=0.1).to(dev)
        if kind == "conv":
            self.pw = ops.pack_conv_weight(bf(rnd("gw", (C, C, 3, 3), std=(9 * C) ** -0.5)), rnd("gb", (C,), std=0.1), dt, dev)
            self.x = bf(rnd("gx", (B, N, C))).to(tdt).to(dev).contiguous()
            self.tiles, self.bias = ops.conv_tiles(self.pw, H, W, dt), self.pw.bias
        elif kind == "proj":
            self.pw = ops.pack_linear_weight(bf(rnd("pw", (C, C), std=C ** -0.5)), rnd("pb", (C,), std=0.1), dt, dev)
            self.x = bf(rnd("px", (B, N, C))).to(tdt).to(dev).contiguous()
            self.tiles, self.bias = 1, self.pw.bias
        else:
            mid, hid = 6, 288
            sd = {"n2.weight": 1 + rnd("hg", (C,), std=0.1), "n2.bias": rnd("hbb", (C,), std=0.1),
                  "m.fc1.weight": bf(rnd("h1w", (2 * hid, C), std=C ** -0.5)), "m.fc1.bias": rnd("h1b", (2 * hid,), std=0.1),
                  "m.dw.weight": rnd("hdw", (2 * hid, 1, 3, 3), std=1 / 3).half().float(), "m.dw.bias": rnd("hdb", (2 * hid,), std=0.1).half().float(),
                  "m.fc2.weight": rnd("h2w", (C, hid), std=hid ** -0.5).half().float(), "m.fc2.bias": rnd("h2b", (C,), std=0.1)}
            self.pw = ops.pack_linear_weight(bf(rnd("hhwa", (C, C), std=C ** -0.5)), rnd("hhba", (C,), std=0.1), dt, dev)
            self.pf = ops.pack_ffn3(sd["m.fc1.weight"], sd["m.fc1.bias"], sd["m.dw.weight"], sd["m.dw.bias"], sd["m.fc2.weight"], sd["m.fc2.bias"],
                                    sd["n2.weight"], sd["n2.bias"], dev)
            self.n2 = (sd["n2.weight"].to(dev), sd["n2.bias"].to(dev))
            self.n = bf(rnd("hhn", (B, N, C))).to(tdt).to(dev).contiguous()
            self.y16 = bf(rnd("hhy", (B, N, 16))).to(tdt).to(dev).contiguous()
            c1 = torch.zeros(B, N, 8)
            c1[..., :mid] = bf(F.gelu(rnd("hhc1", (B, N, mid))))
            self.c1 = c1.to(tdt).to(dev).contiguous()
            self.wf = (torch.randn(B, self.pw.nt * 3 * 512, generator=torch.Generator().manual_seed(5)) * 0.02).to(tdt).to(dev)
            self.bias_b = rnd("hhbb", (B, self.pw.npad), std=0.1).to(dev)
            self.bias = self.pf.b2     # the fc2 bias, fp32: added to the row behind the FFN
            self.tiles = ops.ffn_tiles(self.pf, H, W, dt)

    def run(self, t, in_half, out_half, sat=None, bump=None, pad=0, pad_value=0.0):
        ops, dev, B, H, W, N, dt, tdt = self.ops, self.dev, self.B, self.H, self.W, self.N, self.ops.HAT_BF16, torch.bfloat16
        buf = torch.full((B * N + pad, C), pad_value, dtype=torch.float32)
        buf[:B * N] = t.reshape(B * N, C)
        buf = (buf.half() if in_half else buf).to(dev).contiguous()
        r = buf[:B * N].view(B, N, C)
        out = torch.full((B, N, C), 7.0, dtype=(torch.float16 if out_half else torch.float32), device=dev)
        n = torch.zeros(B, N, C, dtype=tdt, device=dev)
        gap = torch.zeros(B, self.tiles, 16, device=dev)
        n16 = torch.zeros(B, N, 16, dtype=tdt, device=dev)
        kw = {} if sat is None else {"sat": sat}
        if bump is not None:
            kept = self.bias[..., bump[0]].clone()
            self.bias[..., bump[0]] = kept + bump[1]
        try:
            if self.kind == "conv":
                ops.conv(self.pw, self.x, out, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, x_mode=ops.X_NHWC_T, out_mode=ops.O_NHWC_F32, r1=r,
                         ldr1=C, ln=(self.lg, self.lb), ln_out=n, ld_ln=C, gap_out=gap, gap_c=16, n16_out=n16, **kw)
            elif self.kind == "proj":
                ops.linear(self.pw, self.x, out, B=B, H=H, W=W, dtype=dt, ldx=C, ldo=C, out_mode=ops.O_NHWC_F32, r1=r, ldr1=C,
                           ln=(self.lg, self.lb), ln_out=n, ld_ln=C, **kw)
            else:
                ops.hab_tail(self.pf, self.pw, r, out, self.n2[0], self.n2[1], n=self.n, ldn_in=C, y16=self.y16, c1=self.c1, wf=self.wf,
                             bias_b=self.bias_b, B=B, H=H, W=W, dtype=dt, ln1=(self.lg, self.lb), ldn=C, gap_c=16, n_out=n, gap_out=gap,
                             n16_out=n16, **kw)
            torch.cuda.synchronize()
        finally:
            if bump is not None:
                self.bias[..., bump[0]] = kept
        return out.cpu(), n.cpu(), gap.cpu(), n16.cpu()


@pytest.fixture(scope="module")
def drivers():
    made = {}

    def get(kind, geom):
        if (kind, geom) not in made:
            made[(kind, geom)] = Driver(kind, geom, _dev())
        return made[(kind, geom)]
    return get


def slot(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def word(s):
    torch.cuda.synchronize()
    return int(s.cpu()[0]) & 0xFFFFFFFF


def place(d, where):
    """(sample, pixel, channel) of the planted value: an interior tile, the last (ragged) row and column, the 8-byte last n-tile"""
    B, H, W = d.B, d.H, d.W
    return {"interior": (B - 1, 10 * W + 18, 5), "edge": (B - 1, (H - 1) * W + W - 1, 77), "lasttile": (0, 9 * W + 3, 130)}[where]


@pytest.mark.parametrize("in_half", [False, True], ids=["th2", "th3"])
@pytest.mark.parametrize("kind,geom", CASES, ids=IDS)
def test_in_range_changes_nothing(drivers, kind, geom, in_half):
    """In range: the slot stays 0 and every output — rows, LayerNorm rows, pool partials, compact copy — is the unguarded entry's."""
    d = drivers(kind, geom)
    s = slot(d.dev)
    ref = d.run(d.base, in_half, True)
    got = d.run(d.base, in_half, True, sat=s)
    assert float(ref[0].float().abs().max()) < 6e4
    assert word(s) == 0
    assert all(same(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("where", ["interior", "edge", "lasttile"])
@pytest.mark.parametrize("in_half", [False, True], ids=["th2", "th3"])
@pytest.mark.parametrize("kind,geom", CASES, ids=IDS)
def test_one_value_beyond_the_range(drivers, kind, geom, in_half, where):
    """One channel of one pixel inside the image leaves the range: the slot holds the fp32 bit pattern of its magnitude, the rows
    are the unguarded entry's (clamped there).  fp32 rows in: the value is planted in the stream itself.  FP16 rows in cannot
    hold it: the stream holds 65504 there and the launch's fp32 bias lifts that channel by 300 (in range everywhere else)."""
    d = drivers(kind, geom)
    b, p, c = place(d, where)
    t = d.base.clone()
    t[b, p, c], bump = (65504.0, (c, 300.0)) if in_half else (1.3e5, None)
    wide = d.run(t, in_half, False, bump=bump)[0]                # the unguarded entry's fp32 rows: the values before the clamp
    over = wide.abs() > LIM
    assert int(over.sum()) == 1 and bool(over[b, p, c]), "precondition: exactly the planted value is beyond the range"
    ref = d.run(t, in_half, True, bump=bump)
    s = slot(d.dev)
    got = d.run(t, in_half, True, sat=s, bump=bump)
    assert word(s) == bits(wide[b, p, c]), (hex(word(s)), float(wide[b, p, c]))
    assert all(same(a, x) for a, x in zip(got, ref))
    assert float(got[0][b, p, c]) == LIM and same(got[0], wide.clamp(-LIM, LIM).half())


@pytest.mark.parametrize("value", [-1.3e5, float("inf"), float("nan")], ids=["negative", "inf", "nan"])
@pytest.mark.parametrize("kind,geom", [c for c in CASES if c[1][0] == 1], ids=[i for i, c in zip(IDS, CASES) if c[1][0] == 1])
def test_sign_inf_nan_trip(drivers, kind, geom, value):
    d = drivers(kind, geom)
    b, p, c = place(d, "edge")
    t = d.base.clone()
    t[b, p, c] = value
    wide = d.run(t, False, False)[0]
    ref = d.run(t, False, True)
    s = slot(d.dev)
    got = d.run(t, False, True, sat=s)
    if value == -1.3e5:
        assert int((wide.abs() > LIM).sum()) == 1 and word(s) == bits(wide[b, p, c])
        assert float(got[0][b, p, c]) == -LIM
    else:   # an infinity or a NaN among the converted values (the tail's LayerNorm2 turns an infinity into NaNs): at least the infinity's pattern
        assert not torch.isfinite(wide).all() and word(s) >= 0x7F800000
        if torch.isnan(wide).any():
            assert word(s) > 0x7F800000
    assert all(same(a, x) for a, x in zip(got, ref))


def _halo_driver(kind, dev):
    """The ragged 19 x 27 frame with operands that carry a large value ONE PIXEL DOWN AND RIGHT and nowhere else, so that what
    is planted in the frame's last row and column comes out in row H and column W: pixels the tiles compute and never store.
    conv: the only non-zero weights are the identity on the top-left tap, out[y, x] = in[y - 1, x - 1] + bias + r1.
    tail: fc1 takes channel 0 of LayerNorm2(tB) into one hidden unit of each half, the depthwise conv has the top-left tap
    alone, fc2 puts 1000 x that unit into channel 5: out[y, x][5] = tB[y, x][5] + 1000 z^2 sigmoid(z), z = LayerNorm2(tB)[y - 1,
    x - 1][0].  An ordinary pixel has |z| < 5 (under 2.5e4 in all); a pixel whose channel 0 is 3e4 has z = 11.9 (1.4e5)."""
    d = Driver(kind, (1, 19, 27), dev)
    ops, dt = d.ops, d.ops.HAT_BF16
    if kind == "conv":
        w = torch.zeros(C, C, 3, 3)
        w[torch.arange(C), torch.arange(C), 0, 0] = 1.0
        d.pw = ops.pack_conv_weight(w, rnd("gb", (C,), std=0.1), dt, dev)
        d.bias = d.pw.bias
    else:
        hid = 288
        fc1, dw, fc2 = torch.zeros(2 * hid, C), torch.zeros(2 * hid, 1, 3, 3), torch.zeros(C, hid)
        fc1[0, 0] = fc1[hid, 0] = 1.0
        dw[0, 0, 0, 0] = dw[hid, 0, 0, 0] = 1.0
        fc2[5, 0] = 1000.0
        one, zero = torch.ones(C), torch.zeros(C)
        d.pf = ops.pack_ffn3(fc1, torch.zeros(2 * hid), dw, torch.zeros(2 * hid), fc2, zero, one, zero, dev)
        d.n2, d.bias = (one.to(dev), zero.to(dev)), d.pf.b2
    return d


def _halo_plant(d, row, col):
    """the launch's inputs with the large value in frame row `row` and column `col`: (stream, restore)"""
    H, W = d.H, d.W
    t = d.base.clone()
    if d.kind == "conv":   # the conv's bf16 input rows carry it (90112 is a bf16 number)
        x = d.x.clone().view(1, H, W, C)
        x[:, row], x[:, :, col] = 90112.0, 90112.0
        d.x = x.view(1, H * W, C).contiguous()
    else:                  # the stream's channel 0
        tv = t.view(1, H, W, C)
        tv[:, row, :, 0], tv[:, :, col, 0] = 3.0e4, 3.0e4
    return t


@pytest.mark.parametrize("kind", ["tail", "conv"])
def test_no_store_no_trip(kind):
    """A value beyond the range that the kernel computes at pixels it does not store — row H and column W of the ragged tiles —
    does not trip the slot: only the pixels the store predicate admits count.  (The projection walks flat 16-pixel tiles: its
    lanes behind the last pixel recompute the last pixel, there is no pixel of its own there.)  The same operands with the plant
    one row and column earlier bring the value to row H - 1 and column W - 1, inside the frame: then the slot trips, which
    shows that the operands do carry it."""
    dev = _dev()
    d = _halo_driver(kind, dev)
    keep_x = getattr(d, "x", None)
    # (a) planted in the last row and column: computed at row H / column W only
    t = _halo_plant(d, d.H - 1, d.W - 1)
    wide = d.run(t, False, False)[0]
    assert float(wide.abs().max()) <= LIM, "precondition: every stored value is in range"
    ref = d.run(t, False, True)
    s = slot(dev)
    got = d.run(t, False, True, sat=s)
    assert word(s) == 0
    assert all(same(a, x) for a, x in zip(got, ref))
    # (b) planted one earlier: the same values land inside the frame
    d.x = keep_x
    t = _halo_plant(d, d.H - 2, d.W - 2)
    wide = d.run(t, False, False)[0].view(d.H, d.W, C)
    over = wide.abs() > LIM
    assert bool(over[d.H - 1, 1:].any(-1).all()) and bool(over[1:, d.W - 1].any(-1).all()) and not bool(over[:d.H - 1, :d.W - 1].any())
    s = slot(dev)
    d.run(t, False, True, sat=s)
    assert word(s) == bits(wide.abs().max())


def _null_sat(monkeypatch, lib):
    """Every launch of the three unguarded entries goes through its guarded entry with sat == NULL instead; returns the call counts."""
    calls = {}
    for name in ("hat_conv", "hat_linear", "hat_hab_tail3"):
        guarded = getattr(lib, name + "_guarded")

        def shim(desc, stream, guarded=guarded, name=name):
            calls[name] = calls.get(name, 0) + 1
            return guarded(desc, None, stream)
        monkeypatch.setattr(lib, name, shim, raising=False)
    return calls


@pytest.mark.parametrize("in_half", [False, True], ids=["th2", "th3"])
@pytest.mark.parametrize("out_half", [False, True], ids=["f32rows", "f16rows"])
@pytest.mark.parametrize("kind,geom", CASES, ids=IDS)
def test_null_sat_is_the_unguarded_entry(drivers, monkeypatch, kind, geom, in_half, out_half):
    """A guarded entry called with sat == NULL is the unguarded entry, on every descriptor (FP16 or fp32 rows out): every output
    bit for bit, also where the rows are clamped."""
    from super_resolution_amd import _lib
    d = drivers(kind, geom)
    b, p, c = place(d, "edge")
    t = d.base.clone()
    if not in_half:
        t[b, p, c] = -1.3e5
    ref = d.run(t, in_half, out_half)
    calls = _null_sat(monkeypatch, _lib.load())
    got = d.run(t, in_half, out_half)
    assert sum(calls.values()) == 1
    assert all(same(a, x) for a, x in zip(got, ref))


@pytest.mark.parametrize("kind", ["tail", "conv", "proj"])
def test_argument_contract(drivers, kind):
    """sat with fp32 rows out: HAT_EINVAL; a misaligned sat: HAT_EINVAL — on descriptors that launch without it."""
    d = drivers(kind, (1, 19, 27))
    s = torch.zeros(4, dtype=torch.int32, device=d.dev)
    d.run(d.base, False, False)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        d.run(d.base, False, False, sat=s)
    odd = s.view(torch.uint8)[2:6].view(torch.uint8)

    class Odd:   # a slot two bytes off a word boundary, handed to the wrapper as it takes a tensor
        dtype, is_cuda = torch.int32, True
        def numel(self): return 1
        def is_contiguous(self): return True
        def data_ptr(self): return odd.data_ptr()
    d.run(d.base, False, True, sat=s)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        d.run(d.base, False, True, sat=Odd())
    assert word(s) == 0


KW180 = dict(upscale=2, in_chans=3, img_size=64, window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5,
             img_range=1.0, depths=[2], embed_dim=180, num_heads=[6], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")


def test_embed_dim_180_has_no_guard(monkeypatch):
    """embed_dim 180 and the fp32 path have no FP16 stream: no guard, no guarded launch; and the embed_dim-180 tail, on the
    descriptors of a real forward (which launch through hat_hab_tail3), refuses a slot with HAT_EINVAL."""
    from oracle import hat_oracle as O
    from super_resolution_amd import _lib
    from super_resolution_amd.engine import HATEngine, Options
    dev = _dev()
    cfg = O.make_cfg(**KW180)
    sd = synth.synth_state_dict(O.blank_state_dict(cfg), 77)
    x = synth.synth_input(3, (1, 3, 32, 32)).to(dev)
    eng = HATEngine(cfg, sd, dev, "bf16", options=Options(t16_guard="sync"))
    assert [hb.tail for hb in eng.layers[0].habs] == ["fused180"] * 2, "precondition: the forward launches the embed_dim-180 tail"
    assert eng.t16 is False and eng._guard is None and eng.guarded_launches() == []
    y = eng.forward(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and eng.resolve_t16_guard() is True and eng.t16_fallbacks == 0
    cfg144, sd144 = _cfg_sd(False)
    f32 = HATEngine(cfg144, sd144, dev, "f32", options=Options(t16_guard="sync"))
    assert f32.t16 is False and f32._guard is None and f32.guarded_launches() == []
    lib, s, seen = _lib.load(), slot(dev), []
    guarded = lib.hat_hab_tail3_guarded

    def with_slot(desc, stream):
        seen.append(desc._obj.ffn.C)
        return guarded(desc, s.data_ptr(), stream)
    monkeypatch.setattr(lib, "hat_hab_tail3", with_slot, raising=False)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        eng.forward(x)
    torch.cuda.synchronize()
    assert seen == [180] and word(s) == 0


def test_recorded_plan_has_no_guarded_entry():
    """plan.record_plan on a model whose engine launches guarded entries: the recorded call list holds the unguarded ones only."""
    from super_resolution_amd import plan
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    _, sd = _cfg_sd(False)
    net = build_network(dict(type="HAT", compute_dtype="bf16", **KW)).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(_dev())
    eng = net.engine()
    assert eng.t16_guard == "defer" and eng.guarded_launches()
    dims, buffers, calls = plan.record_plan(net, (1, 3, 32, 48))
    names = [n for n, _ in calls]
    assert "hat_hab_tail3" in names and "hat_conv" in names and "hat_linear" in names
    assert not [n for n in names if n.endswith("_guarded")] and set(names) <= set(plan.FN_IDS)
    assert eng.t16_guard == "defer" and eng._guard.pending == 0      # (recorded with the guard off, and the mode is back)


# ------------------------------------------------------------------------------------------------ engine level
KW = dict(upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=24, squeeze_factor=24, conv_scale=0.01, overlap_ratio=0.5,
          img_range=1.0, depths=[2], embed_dim=144, num_heads=[6], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
SCALE = 1.0e5   # what the stream's first value is scaled by: it then runs at a few 1e5


def _cfg_sd(over):
    from oracle import hat_oracle as O
    cfg = O.make_cfg(**KW)
    sd = synth.synth_state_dict(O.blank_state_dict(cfg), 1234)
    if over:
        # The patch-embed LayerNorm would undo a scaled conv_first, so the scale goes to that LayerNorm's affine part: it makes the
        # stream's first value.  The stream's consumer is the LayerNorm `norm` in front of conv_after_body, which divides the scale
        # out again by itself, and the long skip reads conv_first's own (unscaled) output: the image stays O(1) with nothing scaled down.
        for k in ("patch_embed.norm.weight", "patch_embed.norm.bias"):
            sd[k] = sd[k] * SCALE
    return cfg, sd


def _engine(over, **opt):
    from super_resolution_amd.engine import HATEngine, Options
    cfg, sd = _cfg_sd(over)
    return HATEngine(cfg, sd, _dev(), "bf16", options=Options(**opt))


@pytest.fixture(scope="module")
def frame():
    return synth.synth_input(7, (1, 3, 32, 48)).to(_dev())


@pytest.fixture(scope="module")
def over_refs(frame):
    """(the clipped output of the unguarded FP16 stream, the fp32-stream output) of the over-range model, with the preconditions:
    the two differ, and the guard's word reports a peak beyond 65504."""
    from super_resolution_amd import ops
    y_clip = _engine(True, t16_guard="off").forward(frame).cpu()
    y_f32 = _engine(True, no_t16=True).forward(frame).cpu()
    probe = _engine(True, t16_guard="defer")
    assert probe.guarded_launches(), "precondition: the model stores FP16 rows somewhere"
    probe.forward(frame)
    torch.cuda.synchronize()
    peak = ops.read_sat(probe._guard.word())
    print(f"over-range model: stream peak {peak:.4g}; max-abs clipped vs fp32 output {float((y_clip - y_f32).abs().max()):.3e}")
    assert peak > LIM or peak != peak, peak
    assert torch.isfinite(y_f32).all() and not torch.equal(y_clip, y_f32), "precondition: clipping changed the image"
    return y_clip, y_f32


def test_engine_sync_reruns_on_fp32(frame, over_refs):
    y_clip, y_f32 = over_refs
    eng = _engine(True, t16_guard="sync")
    assert eng.t16 and eng.t16_fallbacks == 0
    y = eng.forward(frame).cpu()
    assert torch.equal(y, y_f32)
    assert eng.t16_fallbacks == 1 and eng.t16 is False and eng.t16_peak > LIM and eng.guarded_launches() == []
    y2 = eng.forward(frame).cpu()
    assert torch.equal(y2, y_f32) and eng.t16_fallbacks == 1 and eng.t16_clipped_frames == 0


def test_engine_defer_counts_and_warns(frame, over_refs):
    y_clip, y_f32 = over_refs
    eng = _engine(True, t16_guard="defer")
    y = eng.forward(frame).cpu()
    assert torch.equal(y, y_clip) and eng.t16_fallbacks == 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert eng.resolve_t16_guard() is False
    assert len(seen) == 1 and "peaked at" in str(seen[0].message) and f"{eng.t16_peak:.4g}" in str(seen[0].message)
    assert eng.t16_clipped_frames == 1 and eng.t16_fallbacks == 1 and eng.t16 is False and eng.t16_peak > LIM
    assert torch.equal(eng.forward(frame).cpu(), y_f32)
    assert eng.resolve_t16_guard() is False and eng.t16_fallbacks == 1 and eng.t16_clipped_frames == 1


def test_engine_sync_with_graph(frame, over_refs):
    """use_graph: the fallback frame and the one after it both come from a graph captured again on the fp32 plan."""
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    y_clip, y_f32 = over_refs
    _, sd = _cfg_sd(True)
    net = build_network(dict(type="HAT", compute_dtype="bf16", use_graph=True, **KW)).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(_dev())
    with net.engine().guard_mode("sync"):
        y1 = net(frame).cpu()
        keys1 = list(net._graphs)
        y2 = net(frame).cpu()
    eng = net.engine()
    assert eng.t16_fallbacks == 1 and eng.t16 is False
    assert torch.equal(y1, y_f32) and torch.equal(y2, y_f32)
    assert keys1 == list(net._graphs) and len(keys1) == 1 and keys1[0][2] is False, "one graph, of the fp32 plan, replayed for both"


def test_engine_in_range_all_modes_agree(frame):
    outs = {}
    for mode in ("off", "defer", "sync"):
        eng = _engine(False, t16_guard=mode)
        assert eng.t16 and bool(eng.guarded_launches()) == (mode != "off")
        y = eng.forward(frame).cpu()
        n_ws = eng.ws_allocations
        assert torch.equal(eng.forward(frame).cpu(), y) and eng.ws_allocations == n_ws == 1
        assert eng.resolve_t16_guard() is True and eng.t16_fallbacks == 0 and eng.t16_clipped_frames == 0 and eng.t16
        outs[mode] = y
    assert torch.equal(outs["defer"], outs["off"]) and torch.equal(outs["sync"], outs["off"])


def test_upscale_frames_delivers_fp32_stream_frames():
    """frames.upscale_frames brings every frame to the host: it runs the guard in "sync" mode, so the over-range model's frames
    are the fp32-stream engine's bytes from the first frame on."""
    import numpy as np
    from super_resolution_amd import frames
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    dev = _dev()
    _, sd = _cfg_sd(True)
    net = build_network(dict(type="HAT", compute_dtype="bf16", **KW)).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    src = [(synth.synth_input(40 + i, (1, 3, 32, 48))[0].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).numpy() for i in range(3)]
    ref = _engine(True, no_t16=True)
    want = [ref.forward_u8(torch.from_numpy(a).to(dev).unsqueeze(0))[0].cpu().numpy() for a in src]
    got = list(frames.upscale_frames(net, iter(src)))
    assert net.engine().t16_fallbacks == 1 and net.engine().t16_clipped_frames == 0
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
