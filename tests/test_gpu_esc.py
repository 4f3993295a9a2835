"""ESC on the device: hat_esc_convffn and hat_window_attention_r against fp64 restatements of the same operation on the kernels' own
inputs (tests/esc_ref.py), the whole model against the reference's goldens (tests/golden/esc_*.npz, gen_golden_esc.py), eager
against graph replay, and a reference-style option file through `python -m super_resolution_amd.test`.

Bars: fp32 1e-4 max-abs (the project's fp32 bar) for kernels, intermediates and outputs.  bf16 kernels: helpers.check's bar, the one
the hat_window_attention tests use.  bf16 whole model: per case the reference's own bf16-vs-fp32 PSNR rounded down to a whole dB and
capped at 40, and its max-abs x 1.25, both recorded in esc_surface.json by the generator."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import esc_ref as R
from helpers import check, esc_ffn_sd as _ffn_sd, max_abs, q, rnd
from oracle import hat_oracle as O
from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

MAP = (20, 37)   # 3 x 4 tiles of 8 x 12: ragged in both axes, the last tile column is one pixel wide


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rows(x_bchw, ld, tdt, dev, fill=7.0):
    """(1,C,H,W) -> device (1, H*W, ld) rows of dtype tdt whose pad channels hold `fill` (nothing may read them)."""
    _, c, h, w = x_bchw.shape
    out = torch.full((1, h * w, ld), fill, dtype=tdt, device=dev)
    out[:, :, :c] = x_bchw[0].reshape(c, h * w).t().to(dev).to(tdt)
    return out


def _maps(rows, c, h, w):
    return rows[0, :, :c].float().cpu().t().reshape(1, c, h, w)


def _convffn(dtype, hid, full, dev, b1_mean=0.0, out_f32=False):
    """hat_esc_convffn once on the 20x37 map; full: with the LayerNorm, the residual and the pool.  -> (out maps, fp64 reference,
    partials or None, raw out rows)."""
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = torch.float32 if out_f32 else ops.TORCH_DTYPE[dt]
    h, w = MAP
    sd = _ffn_sd(hid, dtype, b1_mean)
    pf = ops.pack_esc_convffn(sd, "f", dt, dev)
    x, r = rnd(f"x{hid}", (1, 64, h, w)), rnd(f"r{hid}", (1, 64, h, w))
    g, b = rnd("lng", (64,), std=0.1) + 1.0, rnd("lnb", (64,), std=0.1)
    ldx, ldr, ldo = 68, 72, 72
    xr, rr = _rows(x, ldx, torch.float32, dev), _rows(r, ldr, torch.float32, dev)
    out = torch.full((1, h * w, ldo), 7.0, dtype=tdt, device=dev)
    parts = torch.full((1, ops.esc_convffn_tiles(h, w), 16), 7.0, device=dev) if full else None
    ops.esc_convffn(pf, xr, out, B=1, H=h, W=w, dtype=dt, ln=(g.to(dev), b.to(dev)) if full else None, eps=R.LN_EPS,
                    r=rr if full else None, partials=parts, ldx=ldx, ldr=ldr, ldo=ldo)
    torch.cuda.synchronize()
    sd64 = R.d64(sd)
    n = R.layernorm(x.double(), g.double(), b.double()) if full else x.double()
    ref = R.convffn(n, sd64, "f") + (r.double() if full else 0.0)
    assert float((out[0, :, 64:].float() - 7.0).abs().max()) == 0.0, "pad channels written"
    return _maps(out, 64, h, w), ref, parts, out


@pytest.mark.parametrize("full", [False, True], ids=["plain", "ln+r+pool"])
@pytest.mark.parametrize("hid", [80, 128])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_convffn_matches_fp64(dtype, hid, full):
    dev = _dev()
    from super_resolution_amd import ops
    assert ops.esc_convffn_tiles(*MAP) == 12
    got, ref, parts, raw = _convffn(dtype, hid, full, dev)
    check(got, ref, dtype, f"hat_esc_convffn hid {hid}", f32_tol=1e-4)
    if full:
        # the pool partials are the sums of the stored values of channels 0..15 over each tile's pixels
        stored = got[0, :16].double()
        want = torch.stack([stored[:, ty:ty + 8, tx:tx + 12].sum((1, 2)) for ty in range(0, 20, 8) for tx in range(0, 37, 12)])
        assert parts.shape == (1, 12, 16)
        err = float((parts[0].double().cpu() - want).abs().max())
        assert err <= 1e-4 * max(1.0, float(want.abs().max())), err
        got2, _, parts2, raw2 = _convffn(dtype, hid, full, dev)
        assert torch.equal(raw, raw2) and torch.equal(parts, parts2), "two runs differ"


def test_convffn_fp32_output_rows_from_the_bf16_instantiation():
    dev = _dev()
    got, ref, _, _ = _convffn("bf16", 128, True, dev, out_f32=True)
    check(got, ref, "bf16", "hat_esc_convffn bf16 -> fp32 rows")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_convffn_zero_pads_h_not_x(dtype):
    """The depthwise conv pads h with zeros.  With a proj bias around 1, gelu(b1) outside the image would move the border pixels
    by O(1): the kernel must match the zero-padding restatement and be far from the other one."""
    dev = _dev()
    got, ref, _, _ = _convffn(dtype, 80, False, dev, b1_mean=1.0)
    check(got, ref, dtype, "hat_esc_convffn, zero-padded h", f32_tol=1e-4)
    sd64 = R.d64(_ffn_sd(80, dtype, 1.0))
    x = rnd("x80", (1, 64) + MAP).double()
    xp = F.pad(x, (1, 1, 1, 1))   # x zero-padded instead: h outside the image becomes gelu(b1)
    hp = R.gelu(F.conv2d(xp, sd64["f.proj.weight"], sd64["f.proj.bias"]))
    h2 = R.gelu(F.conv2d(hp, sd64["f.dwc.weight"], sd64["f.dwc.bias"], groups=80)) + hp[:, :, 1:-1, 1:-1]
    wrong = F.conv2d(h2, sd64["f.aggr.weight"], sd64["f.aggr.bias"])
    assert max_abs(wrong, ref) > 0.1 and max_abs(got[:, :, 0], wrong[:, :, 0]) > 0.1


def test_convffn_refuses_bad_arguments():
    dev = _dev()
    from super_resolution_amd import ops
    pf = ops.pack_esc_convffn(_ffn_sd(80, "f32"), "f", ops.HAT_F32, dev)
    x = torch.zeros(1, 20 * 37, 64, device=dev)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.esc_convffn(pf, x, x, B=1, H=20, W=37, dtype=ops.HAT_F32)            # in place: the halo would read written rows
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        ops.esc_convffn(pf, x, torch.zeros_like(x), B=1, H=20, W=37, dtype=ops.HAT_F32, ldx=62)
    pf.hid_p = 64
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.esc_convffn(pf, x, torch.zeros_like(x), B=1, H=20, W=37, dtype=ops.HAT_F32)


@pytest.mark.parametrize("hw", [(40, 72), (33, 64)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_window_attention_r_matches_fp64(dtype, hw):
    """heads 4, d 16, a bias table of std 0.5: 40x72 has reflected keys in every edge window on both axes, 33x64 the largest pad
    reflect allows (31) on one axis and none on the other."""
    dev = _dev()
    from super_resolution_amd import ops
    dt = ops.DTYPE_CODE[dtype]
    tdt = ops.TORCH_DTYPE[dt]
    h, w = hw
    qkv = q(rnd(f"qkv{hw}", (1, 192, h, w)), dtype)
    table = rnd("rpb32", (4, 63 * 63), std=0.5)
    rows = _rows(qkv, 192, tdt, dev)
    rows[:, :, :64] = (rows[:, :, :64].float() * 0.25).to(tdt)   # q pre-multiplied by head_dim^-0.5: a power of two, exact
    out = torch.full((1, h * w, 72), 7.0, dtype=tdt, device=dev)
    ops.window_attention_r(rows, rows.view(-1)[64:], table.to(dev), out, B=1, h=h, w=w, C_=64, heads=4, ws=32, ldq=192, ldkv=192, ldo=72,
                           dtype=dt)
    torch.cuda.synchronize()
    Hp, Wp = -(-h // 32) * 32, -(-w // 32) * 32
    padded = qkv.double()[:, :, R.reflect_index(h, Hp)][:, :, :, R.reflect_index(w, Wp)]
    ref = R.attention_core(padded, table.double(), 32, 4)[:, :, :h, :w]
    check(_maps(out, 64, h, w), ref, dtype, f"hat_window_attention_r {hw}", f32_tol=1e-4)
    assert float((out[0, :, 64:].float() - 7.0).abs().max()) == 0.0, "pad channels written"


def test_window_attention_r_refusals():
    dev = _dev()
    from super_resolution_amd import ops
    z = torch.zeros(1, 16 * 40, 192, device=dev)
    o, t = torch.zeros(1, 16 * 40, 64, device=dev), torch.zeros(4, 63 * 63, device=dev)
    kw = dict(B=1, C_=64, heads=4, ldq=192, ldkv=192, ldo=64, dtype=ops.HAT_F32)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):     # 16 rows cannot be reflect-padded to 32
        ops.window_attention_r(z, z.view(-1)[64:], t, o, h=16, w=40, ws=32, **kw)
    with pytest.raises(RuntimeError, match="HAT_EUNSUPPORTED"):
        ops.window_attention_r(z, z.view(-1)[64:], t, o, h=16, w=40, ws=16, **kw)


def test_esc_layernorm_eps_and_shuffle_add():
    dev = _dev()
    from super_resolution_amd import ops
    x = rnd("lnx", (1, 64, 5, 7), std=1e-3)   # small rows: eps 1e-6 against 1e-5 is a visible difference
    g, b = rnd("lng", (64,), std=0.1) + 1.0, rnd("lnb", (64,), std=0.1)
    xr = _rows(x, 64, torch.float32, dev)
    y = torch.zeros(1, 35, 64, device=dev)
    ops.esc_layernorm(xr, y, g.to(dev), b.to(dev), npix=35, dtype=ops.HAT_F32, eps=1e-6)
    check(_maps(y, 64, 5, 7), R.layernorm(x.double(), g.double(), b.double(), 1e-6), "f32", "hat_esc_layernorm", f32_tol=1e-4)
    assert max_abs(R.layernorm(x.double(), g.double(), b.double(), 1e-5), R.layernorm(x.double(), g.double(), b.double(), 1e-6)) > 0.1
    for s in (2, 3, 4):
        ld = (3 * s * s + 3) // 4 * 4
        rows, img = rnd(f"sh{s}", (1, 3 * s * s, 5, 7)), rnd("shx", (1, 3, 5, 7))
        out = torch.zeros(1, 3, 5 * s, 7 * s, device=dev)
        ops.esc_shuffle_add(_rows(rows, ld, torch.float32, dev), img.to(dev), out, B=1, H=5, W=7, s=s, ld=ld)
        assert torch.equal(out.cpu(), F.pixel_shuffle(rows + torch.repeat_interleave(img, s * s, dim=1), s))


# ---- whole model ------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name, dtype, dev):
    """The ESC of golden case `name` with its seeded weights ('c': case a converted; 'd': case a's checkpoint in a x3 model)."""
    from super_resolution_amd.registry import build_network
    if (name, dtype) not in _NETS:
        cfg, sd, g, meta = R.load_case(name)
        net = build_network(dict(cfg, type="ESC", attn_type="Naive", compute_dtype=dtype)).eval()
        net.load_state_dict(sd, strict=True)
        if name == "c":
            net.convert()
        _NETS[(name, dtype)] = (net.to(dev), g, meta)
    return _NETS[(name, dtype)]


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_whole_model_fp32_matches_reference(name):
    dev = _dev()
    net, g, _ = _net(name, "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    taps = {}
    y = net.engine(dev).forward(x, taps=taps).clone()
    if "tap_pixels" in g:   # the intermediates first, so that a failure points at a stage
        px = torch.from_numpy(g["tap_pixels"])
        for k in R.TAPS:
            err = max_abs(taps[k][0].cpu()[px], g[k])
            print(f"esc_{name} {k}: max-abs {err:.3e}")
            assert err <= 1e-4, f"esc_{name} {k}: max-abs {err:.3e}"
    err = max_abs(y.cpu(), g["y"])
    print(f"esc_{name} y: max-abs {err:.3e}")
    assert err <= 1e-4, f"esc_{name}: max-abs {err:.3e}"
    assert torch.equal(net(x), y)


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_whole_model_bf16_within_the_reference_bf16_deviation(name):
    dev = _dev()
    net, g, meta = _net(name, "bf16", dev)
    y = net(torch.from_numpy(g["x"]).to(dev)).cpu()
    psnr, err = O.psnr_float(y, torch.from_numpy(g["y"])), max_abs(y, g["y"])
    bar_db, bar_abs = min(40.0, math.floor(meta["bf16"]["psnr"])), 1.25 * meta["bf16"]["max_abs"]
    print(f"esc_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})")
    assert psnr >= bar_db and err <= bar_abs, f"esc_{name} bf16: PSNR {psnr:.2f} dB (bar {bar_db}), max-abs {err:.4f} (bar {bar_abs:.4f})"


def test_graph_replay_equals_eager_and_second_size():
    dev = _dev()
    net, g, _ = _net("a", "fp32", dev)
    x = torch.from_numpy(g["x"]).to(dev)
    eager = net(x)
    net.use_graph = True
    try:
        assert torch.equal(net(x), eager) and torch.equal(net(x), eager)   # capture, then replay
        x2 = synth.synth_input(R.X_SEED, (1, 3, 33, 64)).to(dev)           # another size after 40x72: the workspace is keyed by shape
        cfg, sd, _, _ = R.load_case("a")
        want = R.forward(R.d64(sd), cfg, x2.cpu().double())
        assert max_abs(net(x2).cpu(), want) <= 1e-4
        assert torch.equal(net(x), eager)
    finally:
        net.use_graph = False
    assert max_abs(net(x2).cpu(), want) <= 1e-4 and torch.equal(net(x), eager)


def test_batch_and_small_frames_are_refused():
    dev = _dev()
    net, _, _ = _net("a", "fp32", dev)
    with pytest.raises(RuntimeError, match="one frame"):
        net(torch.zeros(2, 3, 40, 40, device=dev))
    with pytest.raises(RuntimeError, match="reflect-padded"):
        net(torch.zeros(1, 3, 16, 40, device=dev))


def _fresh_engine(dev):
    """A new engine (empty workspace cache, its own lock) over case a's network: n_blocks 1, conv_blocks 1, fp32."""
    from super_resolution_amd.esc_engine import ESCEngine
    net, _, _ = _net("a", "fp32", dev)
    return ESCEngine(net.cfg, net.state_dict(), dev, "fp32")


def test_engine_refuses_host_and_other_device_tensors_before_any_launch():
    dev = _dev()
    eng = _fresh_engine(dev)
    x = synth.synth_input(R.X_SEED, (1, 3, 33, 40)).to(dev)
    with pytest.raises(RuntimeError, match="device tensor"):
        eng.forward(x.cpu())
    if torch.cuda.device_count() >= 2:
        with pytest.raises(RuntimeError, match="lives on"):
            eng.forward(x.to("cuda:1"))
    assert len(eng._ws_cache) == 0 and eng.ws_allocations == 0


def test_one_forward_at_a_time_per_engine():
    """Three threads on one engine, two of them on the same shape, so on the same workspace (w["s"], w["gap"], w["weff"] and the
    output buffer): every result, cloned under no lock of the thread's own, is the serial one bit for bit."""
    import threading
    dev = _dev()
    eng = _fresh_engine(dev)
    x33, x40 = (synth.synth_input(R.X_SEED + i, shape).to(dev) for i, shape in enumerate([(1, 3, 33, 40), (1, 3, 40, 33)]))
    y33, y40 = eng.forward(x33).clone(), eng.forward(x40).clone()
    got, errors = [], []

    def run(x, want):
        try:
            for _ in range(8):
                got.append((eng.forward(x).clone(), want))
        except Exception as e:   # noqa: BLE001  (reported by the assert below, with the thread's traceback text)
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=a, daemon=True) for a in ((x33, y33), (x40, y40), (x33, y33))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a forward did not come back within 60 s"
    assert not errors, errors
    assert len(got) == 24 and all(torch.equal(y, want) for y, want in got)


def test_reference_style_yaml_through_the_test_entry(tmp_path):
    """An option file as the reference ships them (model_type ESRModel, network_g.type ESC) through `python -m
    super_resolution_amd.test`: the PSNR is the one metrics.py gives for the fp32 golden path's output (tests/esc_ref.py in fp32 on
    the host), within 1e-3 dB."""
    dev = _dev()
    import yaml
    from super_resolution_amd import data as D, metrics as M, test as T
    cfg, sd, _, _ = R.load_case("a")
    torch.save({"params": sd}, tmp_path / "net.pth")
    sizes = [(40, 45), (36, 50)]
    for i, (h, w) in enumerate(sizes):
        D.write_image(M.tensor2img(synth.synth_input(30 + i, (1, 3, h, w))), str(tmp_path / "lq" / f"im{i}.png"))
        D.write_image(M.tensor2img(synth.synth_input(40 + i, (1, 3, 2 * h, 2 * w))), str(tmp_path / "gt" / f"im{i}.png"))
    opt = {"name": "ESC_toy_X2", "model_type": "ESRModel", "scale": 2, "num_gpu": 1,
           "datasets": {"test_1": {"name": "Toy", "type": "PairedImageDataset", "dataroot_gt": str(tmp_path / "gt"),
                                   "dataroot_lq": str(tmp_path / "lq"), "io_backend": {"type": "disk"}}},
           "network_g": dict(cfg, type="ESC", attn_type="Naive", compute_dtype="fp32"),
           "path": {"pretrain_network_g": str(tmp_path / "net.pth"), "strict_load_g": True, "param_key_g": "params",
                    "visualization": str(tmp_path / "vis")},
           "val": {"save_img": False, "suffix": None, "metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 2, "test_y_channel": True}}}}
    (tmp_path / "opt.yml").write_text(yaml.safe_dump(opt))
    res = T.main(["-opt", str(tmp_path / "opt.yml")])
    rows = {r.get("name", r.get("img_name", i)): r for i, r in enumerate(res["Toy"]["images"])}
    assert len(rows) == 2
    for i, (h, w) in enumerate(sizes):
        lq = D.read_image(str(tmp_path / "lq" / f"im{i}.png")).unsqueeze(0)
        xp = F.pad(lq, (0, (-w) % 32, 0, (-h) % 32), "reflect")
        y = R.forward(sd, cfg, xp)[:, :, :2 * h, :2 * w]
        gt8 = M.tensor2img(D.read_image(str(tmp_path / "gt" / f"im{i}.png")))
        want = M.calculate_metric({"img": M.tensor2img(y), "img2": gt8}, opt["val"]["metrics"]["psnr"])
        assert res["Toy"]["images"][i]["psnr"] == pytest.approx(want, abs=1e-3)
