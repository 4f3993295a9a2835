"""The geometric self-ensemble without a GPU: the oracle driven through the tests' restatement of the eight-member loop
(ensemble_ref.py) against goldens made with the reference's network (tests/golden/gen_golden_ensemble.py); the argument contract
of hat_dihedral_f32 (every check returns before a launch); the option plumbing of the harness and the two command lines."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

import ensemble_ref as E
from helpers import META, W_SEED, X_SEED, golden, max_abs, oracle_sd
from oracle import hat_oracle as O
from super_resolution_amd import synth

EINVAL = -1   # include/hat_mi355x.h
CASES = {"tiny_x2": (1, 3, 16, 24), "tiny_x4": (1, 3, 24, 16), "hats_1g_x4": (1, 3, 16, 32)}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_ensemble_matches_the_reference_goldens(name):
    """<= 1e-5 max-abs, the project's oracle bar, for the ensembles of eight and of four; the members themselves differ by
    about 3 (the generator prints the smallest pairwise distance), so a wrong transform cannot pass."""
    g = golden(f"ensemble_{name}.npz")
    assert tuple(g["x_shape"]) == CASES[name]
    cfg, sd = oracle_sd(name)
    x = synth.synth_input(X_SEED, CASES[name])
    outs = E.member_outputs(lambda t: O.hat_forward(t, sd, cfg), x, 8)
    s = cfg["upscale"]
    for n in (8, 4):
        y = E.accumulate(outs, n)
        assert y.shape == (1, 3, s * x.shape[2], s * x.shape[3])
        err = max_abs(y, g[f"y{n}"])
        print(f"ENSEMBLE-ORACLE {name} n={n}: max-abs vs golden {err:.3e}")
        assert err <= 1e-5, (name, n, err)
    sep = min(max_abs(outs[a], outs[b]) for a in range(8) for b in range(a))
    assert sep > 1.0, f"the members are {sep} apart: the goldens would not tell them apart"
    assert max_abs(g["y8"], g["y4"]) > 1e-2


def test_hatx_oracle_through_the_loop():
    cfg = O.make_hatx_cfg(**META["cfgs"]["hatx_tiny_plain_x2"])
    sd = synth.synth_state_dict(O.hatx_blank_state_dict(cfg), W_SEED)
    x = synth.synth_input(X_SEED, (1, 3, 16, 24))
    net = lambda t: O.hatx_forward(t, sd, cfg)
    y = E.ensemble(net, x, 8)
    assert y.shape == (1, 3, 32, 48) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    assert torch.equal(E.ensemble(net, x, 1), net(x))


@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


def test_dihedral_refuses_bad_arguments(lib):
    src, dst = C.c_void_p(0x10000), C.c_void_p(0x90000)     # distinct non-null addresses 512 KiB apart: never dereferenced on the host
    call = lambda s=src, d=dst, planes=3, H=16, W=24, op=0, inv=0, acc=0: lib.hat_dihedral_f32(s, d, planes, H, W, op, inv, 1.0, acc, None)
    assert call(s=None) == EINVAL and call(d=None) == EINVAL
    for op in (-1, 8, 9, 64):
        assert call(op=op) == EINVAL and call(op=op, inv=1) == EINVAL
    for bad in (dict(planes=0), dict(planes=-1), dict(H=0), dict(W=0), dict(H=-5), dict(W=-5)):
        assert call(**bad) == EINVAL, bad
    # the grid: planes on z, 64-wide tiles of either axis on x / y
    assert call(planes=65536, H=1, W=1) == EINVAL
    assert call(planes=1, H=65535 * 64 + 1, W=1) == EINVAL and call(planes=1, H=1, W=65535 * 64 + 1) == EINVAL
    # overlapping ranges, for every member (a transposing one in place would read cells it has written): 3 * 16 * 24 floats = 4608 B
    for op in range(8):
        assert call(d=src, op=op) == EINVAL
        assert call(d=C.c_void_p(0x10000 + 4604), op=op) == EINVAL and call(s=C.c_void_p(0x10000 + 4604), d=src, op=op) == EINVAL
    big = 0x10000 + 4 * 64 * 4096 * 4096 - 4      # the byte count of a large block is computed in 64 bits: 4 GiB, not 0
    assert call(d=C.c_void_p(big), planes=64, H=4096, W=4096) == EINVAL


def test_ensemble_members_option():
    from super_resolution_amd import ops
    from super_resolution_amd.models import HATModel
    for n in (1, 2, 4, 8):
        assert ops.ensemble_members(n) == n
    for bad in (0, 3, 5, 6, 7, 16, -8, True, False, None, "8", 8.0):
        with pytest.raises(ValueError):
            ops.ensemble_members(bad)
    f = HATModel.self_ensemble_members
    assert (f(True), f(2), f(4), f(8)) == (8, 2, 4, 8)
    assert f(None) == 1 and f(False) == 1          # the option is off
    for bad in (0, 1, 3, 6, 16, -2, "8", "true", 8.0, [8]):
        with pytest.raises(ValueError):
            f(bad)


def test_test_cli_parses_self_ensemble(tmp_path, monkeypatch):
    from super_resolution_amd import test as T
    opt = {"name": "toy", "scale": 2, "network_g": {"type": "HAT"}, "val": {"save_img": False, "suffix": None}}
    yml = tmp_path / "opt.yml"
    yml.write_text(yaml.safe_dump(opt))
    assert "self_ensemble" not in T.parse_options(str(yml))["val"]
    assert T.parse_options(str(yml), self_ensemble=4)["val"] == {"save_img": False, "suffix": None, "self_ensemble": 4}
    seen = []

    class Model:
        def __init__(self, opt, device=None):
            seen.append(opt)

    monkeypatch.setattr(T, "HATModel", Model)
    for argv, want in (([], None), (["--self-ensemble"], 8), (["--self-ensemble", "2"], 2), (["--self-ensemble", "4", "--u8"], 4),
                       (["--self-ensemble", "8"], 8)):
        T.main(["-opt", str(yml)] + argv)
        assert (seen[-1].get("val") or {}).get("self_ensemble") == want, argv
    assert seen[-2]["val"]["u8_on_device"] is True
    for bad in ("1", "3", "16", "all"):
        with pytest.raises(SystemExit):
            T.main(["-opt", str(yml), "--self-ensemble", bad])
    # a YAML value the harness does not know is refused by the harness, before the first image
    from super_resolution_amd.models import HATModel
    m = HATModel.__new__(HATModel)
    m.opt = {"val": {"self_ensemble": 3}}
    with pytest.raises(ValueError, match="self_ensemble"):
        m.nondist_validation(type("D", (), {"opt": {"name": "x"}})(), save_img=False)


def test_video_cli_parses_self_ensemble(tmp_path, monkeypatch):
    from super_resolution_amd import frames, video, y4m
    base = ["-opt", "o.yml", "-i", "a.y4m", "-o", "b.y4m"]
    assert video.parser().parse_args(base).self_ensemble is None         # main hands `or 1` to upscale_file
    assert video.parser().parse_args(base + ["--self-ensemble"]).self_ensemble == 8
    assert video.parser().parse_args(base + ["--self-ensemble", "4"]).self_ensemble == 4
    for bad in ("1", "3", "0", "many"):                                     # the same choices as the test CLI: 2, 4, 8
        with pytest.raises(SystemExit):
            video.parser().parse_args(base + ["--self-ensemble", bad])
    import inspect
    assert "ensemble=args.self_ensemble or 1" in inspect.getsource(video.main)
    hdr = {"W": 6, "H": 4, "F": "24:1", "I": "p", "A": "1:1", "C": "420jpeg", "X": []}
    with y4m.Writer(str(tmp_path / "in.y4m"), hdr) as wr:
        wr.write(np.zeros((6, 6), dtype=np.uint8))
    calls = []

    class Net:
        upscale = 2

    def fake(net, it, **kw):
        calls.append(kw)
        for a in it:
            yield np.repeat(np.repeat(a, 2, 0), 2, 1)

    monkeypatch.setattr(frames, "upscale_frames", fake)
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), ensemble=8)
    assert info["ensemble"] == 8 and calls[-1]["ensemble"] == 8
    info = video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"))
    assert "ensemble" not in info and "ensemble" not in calls[-1]
    with pytest.raises(ValueError):
        video.upscale_file(Net(), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), ensemble=3)
