"""PSNR / SSIM on the device, the parts that need no GPU: the two C entry points are declared, bound and exported;
hat_u8_metrics and its workspace query refuse bad arguments before they touch the device; `metrics_device.finalize` is plain
host arithmetic; `--metrics-on-device` sets the two `val` keys and its absence leaves the parsed options alone."""
import ctypes as C
import math
import os
import re

import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hat_mi355x.h")
EINVAL = -1
Y, BGR, PSNR, SSIM = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lib():
    from super_resolution_amd import _lib, build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    """Host memory standing in for device pointers: a call that is refused never dereferences them."""
    return C.create_string_buffer(4096)


def test_both_entry_points_are_declared_bound_and_exported(lib):
    from super_resolution_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = C.CDLL(build.LIB)
    for name in ("hat_u8_metrics", "hat_u8_metrics_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/hat_mi355x.h"
        assert name in _lib.SIGNATURES
        assert getattr(raw, name, None) is not None, f"{name} is not exported"
    for flag, value in (("HAT_METRICS_Y", Y), ("HAT_METRICS_BGR", BGR), ("HAT_METRICS_PSNR", PSNR), ("HAT_METRICS_SSIM", SSIM)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (flag, value), src), flag
    assert (_lib.METRICS_Y, _lib.METRICS_BGR, _lib.METRICS_PSNR, _lib.METRICS_SSIM) == (Y, BGR, PSNR, SSIM)
    assert "hat_metrics.hip" in build.SOURCES
    assert lib.hat_abi_version() == 2


def _query(lib, B, h, w, crop, flags):
    n = C.c_int64(-1)
    rc = lib.hat_u8_metrics_workspace_bytes(B, h, w, crop, flags, C.byref(n))
    return rc, n.value


def test_u8_metrics_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem) // 8 * 8 + 8
    ok = dict(a=p, apitch=3 * 40, abs=3 * 40 * 30, b=p, bpitch=3 * 40, bbs=3 * 40 * 30, B=1, h=30, w=40, crop=4, flags=Y | PSNR | SSIM,
              sums=p, ws=p)
    call = lambda **kw: lib.hat_u8_metrics(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("a", "b", "sums", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(apitch=3 * 40 - 1) == EINVAL and call(bpitch=3 * 40 - 1) == EINVAL      # a row does not fit its pitch
    assert call(B=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL and call(crop=-1) == EINVAL
    assert call(B=2, abs=3 * 40 * 29) == EINVAL and call(B=2, bbs=3 * 40 * 29) == EINVAL  # samples overlap
    assert call(flags=Y) == EINVAL                                                      # neither metric selected
    assert call(flags=PSNR | 16) == EINVAL                                              # an unknown flag bit
    assert call(h=18) == EINVAL and call(w=18) == EINVAL                                 # 10 x 32 / 22 x 10 after the crop: no 11x11 window
    assert call(h=8, flags=PSNR) == EINVAL and call(w=8, flags=Y | PSNR) == EINVAL         # nothing is left of the frame


def test_workspace_query_applies_the_same_size_rules(lib):
    for flags in (Y | SSIM, SSIM, Y | PSNR | SSIM, PSNR | SSIM | BGR):
        assert _query(lib, 1, 12, 12, 1, flags)[0] == EINVAL                            # 10 x 10 after the crop
        assert _query(lib, 1, 13, 12, 1, flags)[0] == EINVAL and _query(lib, 1, 12, 13, 1, flags)[0] == EINVAL
        rc, n = _query(lib, 1, 13, 13, 1, flags)                                        # 11 x 11: one SSIM position
        assert rc == 0 and n > 0
    assert _query(lib, 1, 12, 12, 1, PSNR)[0] == 0                                      # PSNR alone needs a pixel, not a window
    assert _query(lib, 1, 2, 12, 1, PSNR)[0] == EINVAL and _query(lib, 1, 12, 2, 1, Y | PSNR)[0] == EINVAL
    assert _query(lib, 0, 13, 13, 1, SSIM)[0] == EINVAL and _query(lib, 1, 13, 13, -1, SSIM)[0] == EINVAL
    assert _query(lib, 1, 13, 13, 1, Y)[0] == EINVAL and _query(lib, 1, 13, 13, 1, SSIM | 32)[0] == EINVAL
    assert lib.hat_u8_metrics_workspace_bytes(1, 13, 13, 1, SSIM, None) == EINVAL
    assert _query(lib, 1, 11, 11, 0, SSIM)[0] == 0 and _query(lib, 1, 10, 11, 0, SSIM)[0] == EINVAL   # crop_border 0 crops nothing


def test_workspace_for_the_headline_frame_and_monotone_growth(lib):
    for flags in (Y | PSNR | SSIM, PSNR | SSIM):
        rc, base = _query(lib, 1, 2880, 5120, 4, flags)
        assert rc == 0 and 0 < base < 64 << 20
        for B, h, w in ((2, 2880, 5120), (1, 2881, 5120), (1, 2880, 5121), (1, 4000, 5120), (1, 2880, 8000), (3, 3000, 6000)):
            rc, n = _query(lib, B, h, w, 4, flags)
            assert rc == 0 and n >= base, (B, h, w)
    sizes = [_query(lib, 1, s, s, 0, Y | PSNR | SSIM) for s in range(11, 700, 13)]
    assert all(rc == 0 for rc, _ in sizes)
    assert [n for _, n in sizes] == sorted(n for _, n in sizes)


def test_finalize_on_hand_made_sums():
    from super_resolution_amd.metrics_device import finalize
    h, w, cb = 40, 50, 3
    hc, wc = h - 2 * cb, w - 2 * cb
    pos = (hc - 10) * (wc - 10)
    r = finalize([0.0, 0.5 * pos, 0.0, 0.0], h, w, cb, True)
    assert r["psnr"] == float("inf") and r["ssim"] == pytest.approx(0.5, rel=1e-15)
    sse = 123457.0
    r = finalize([sse, 0.25 * pos, 0.5 * pos, 0.75 * pos], h, w, cb, False)            # RGB: three channels
    assert r["psnr"] == pytest.approx(10.0 * math.log10(255.0 ** 2 * (hc * wc * 3) / sse), rel=1e-15)
    assert r["ssim"] == pytest.approx(0.5, rel=1e-15)                                   # the mean of the three channel means
    r = finalize([sse, 0.25 * pos, 0.5 * pos, 0.75 * pos], h, w, cb, True)             # Y: one channel, entries 2 and 3 are not read
    assert r["psnr"] == pytest.approx(10.0 * math.log10(255.0 ** 2 * (hc * wc) / sse), rel=1e-15)
    assert r["ssim"] == pytest.approx(0.25, rel=1e-15)
    r = finalize([7.0, 3.0 * 30 * 40, 0, 0], 40, 50, 0, True)                            # crop_border 0
    assert r["psnr"] == pytest.approx(10.0 * math.log10(255.0 ** 2 * 2000 / 7.0), rel=1e-15) and r["ssim"] == pytest.approx(3.0, rel=1e-15)
    assert isinstance(r["psnr"], float) and isinstance(r["ssim"], float)


def test_metrics_on_device_flag_sets_both_keys_and_nothing_else(tmp_path):
    from super_resolution_amd import test as T
    opt = {"name": "toy", "scale": 2, "datasets": {"test_1": {"name": "Toy", "dataroot_lq": "lq"}}, "network_g": {"type": "HAT"},
           "val": {"save_img": False, "suffix": None}}
    yml = tmp_path / "opt.yml"
    yml.write_text(yaml.safe_dump(opt))
    parent = dict(yaml.safe_load(yml.read_text()), is_train=False)       # what the parser makes of the YAML without a flag
    parent["datasets"]["test_1"].update(phase="test", scale=2)
    assert T.parse_options(str(yml)) == parent
    assert T.parse_options(str(yml), metrics_on_device=False) == parent
    with_flag = T.parse_options(str(yml), metrics_on_device=True)
    assert with_flag["val"] == {"save_img": False, "suffix": None, "u8_on_device": True, "metrics_on_device": True}
    assert {k: v for k, v in with_flag.items() if k != "val"} == {k: v for k, v in parent.items() if k != "val"}
    assert "metrics_on_device" not in T.parse_options(str(yml), u8=True)["val"]
    noval = tmp_path / "noval.yml"
    noval.write_text(yaml.safe_dump({k: v for k, v in opt.items() if k != "val"}))
    assert T.parse_options(str(noval), metrics_on_device=True)["val"] == {"u8_on_device": True, "metrics_on_device": True}
    import inspect  # the command line carries the flag through to parse_options
    assert '"--metrics-on-device"' in inspect.getsource(T.main) and "metrics_on_device=args.metrics_on_device" in inspect.getsource(T.main)
