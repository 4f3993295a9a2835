"""The 8-bit frame boundary without a GPU: hat_u8_to_planes, hat_planes_to_u8, hat_conv3x3_to_u8 and hat_plan_forward_u8
check their arguments before they touch the device; the PPM example is plain C; `--u8` sets val.u8_on_device and its
absence leaves the parsed options alone."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


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


def test_u8_to_planes_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem)
    ok = dict(src=p, pitch=3 * 20, bstride=3 * 20 * 10, dst=p, B=1, h=10, w=20, Hp=16, Wp=32, bgr=0)
    call = lambda **kw: lib.hat_u8_to_planes(*[dict(ok, **kw)[k] for k in ok], None)
    assert call(src=None) == EINVAL and call(dst=None) == EINVAL
    assert call(B=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(pitch=3 * 20 - 1) == EINVAL                   # a row does not fit its pitch
    assert call(Hp=9) == EINVAL and call(Wp=19) == EINVAL      # the padded plane is smaller than the frame
    assert call(Hp=20) == EINVAL and call(Wp=40) == EINVAL     # padding == size: nothing left to reflect
    assert call(h=1, Hp=2) == EINVAL
    assert call(B=2, bstride=3 * 20 * 9) == EINVAL             # samples overlap


def test_planes_to_u8_rejects_bad_arguments(lib, mem):
    p = C.addressof(mem)
    ok = dict(src=p, B=1, Hs=16, Ws=32, dst=p, pitch=3 * 30, bstride=3 * 30 * 12, h=12, w=30, bgr=0)
    call = lambda **kw: lib.hat_planes_to_u8(*[dict(ok, **kw)[k] for k in ok], None)
    assert call(src=None) == EINVAL and call(dst=None) == EINVAL
    assert call(B=0) == EINVAL and call(Hs=0) == EINVAL and call(Ws=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(pitch=3 * 30 - 1) == EINVAL
    assert call(h=17) == EINVAL and call(w=33, pitch=99) == EINVAL   # the crop reaches outside the planes
    assert call(B=2, bstride=3 * 30 * 11) == EINVAL


def test_conv3x3_to_u8_rejects_bad_arguments(lib, mem):
    from super_resolution_amd import _lib
    p = C.addressof(mem) // 16 * 16 + 16
    mean = (C.c_float * 4)(0.4488, 0.4371, 0.4040, 0.0)
    ok = dict(x=p, wpk=p, bias=p, dst=p, pitch=3 * 30, bstride=3 * 30 * 12, B=1, H=16, W=32, Cc=64, ldx=64, h=12, w=30, scale=1.0,
              mean=mean, bgr=0, dtype=_lib.HAT_BF16)
    call = lambda **kw: lib.hat_conv3x3_to_u8(*[dict(ok, **kw)[k] for k in ok], None)
    for k in ("x", "wpk", "bias", "dst", "mean"):
        assert call(**{k: None}) == EINVAL, k
    assert call(B=0) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL and call(h=0) == EINVAL and call(w=0) == EINVAL
    assert call(W=40) == EINVAL                                 # the row sweep needs W % 16 == 0
    assert call(pitch=3 * 30 - 1) == EINVAL
    assert call(h=17) == EINVAL and call(w=33, pitch=99) == EINVAL
    assert call(x=p + 2) == EINVAL                              # fragment loads are 16-byte aligned
    assert call(dtype=_lib.HAT_F32) == -3 and call(Cc=48) == -3  # HAT_EUNSUPPORTED: only the bf16 conv_last shape is built


def test_plan_forward_u8_rejects_bad_arguments(lib, mem):
    """Null pointers, zero sizes and a source pitch below 3 w.  The undefined reflection (H - h >= h), a frame larger than the
    plan and a destination pitch below 3 s w are measured against the plan's shape, and a plan cannot be loaded without a
    device: tests/test_gpu_u8.py::test_plan_forward_u8 checks those three on a loaded plan."""
    p = C.addressof(mem)
    assert lib.hat_plan_forward_u8(None, p, 60, 10, 20, p, 240, 0, None) == EINVAL
    # the checks that need no plan come before the plan is read: a stand-in handle is never dereferenced
    assert lib.hat_plan_forward_u8(p, None, 60, 10, 20, p, 240, 0, None) == EINVAL
    assert lib.hat_plan_forward_u8(p, p, 60, 10, 20, None, 240, 0, None) == EINVAL
    assert lib.hat_plan_forward_u8(p, p, 60, 0, 20, p, 240, 0, None) == EINVAL
    assert lib.hat_plan_forward_u8(p, p, 60, 10, 0, p, 240, 0, None) == EINVAL
    assert lib.hat_plan_forward_u8(p, p, 59, 10, 20, p, 240, 0, None) == EINVAL


def test_ppm_example_is_plain_c(tmp_path):
    """examples/plan_upscale_u8.c compiles as C (not C++) and links against the library and the HIP runtime with gcc alone."""
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from super_resolution_amd import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    exe = tmp_path / "plan_upscale_u8"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", os.path.join(ROOT, "examples", "plan_upscale_u8.c"), "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(ROOT, "super_resolution_amd"), "-lhat_mi355x",
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "super_resolution_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(exe)


def test_u8_flag_sets_the_key_and_nothing_else(tmp_path):
    from super_resolution_amd import test as T
    opt = {"name": "toy", "scale": 2, "datasets": {"test_1": {"name": "Toy", "dataroot_lq": "lq"}}, "network_g": {"type": "HAT"},
           "val": {"save_img": False, "suffix": None}}
    yml = tmp_path / "opt.yml"
    yml.write_text(yaml.safe_dump(opt))
    parent = dict(yaml.safe_load(yml.read_text()), is_train=False)       # what the parser did before the flag existed
    parent["datasets"]["test_1"].update(phase="test", scale=2)
    assert T.parse_options(str(yml)) == parent
    assert "u8_on_device" not in T.parse_options(str(yml))["val"]
    with_flag = T.parse_options(str(yml), u8=True)
    assert with_flag["val"] == {"save_img": False, "suffix": None, "u8_on_device": True}
    assert {k: v for k, v in with_flag.items() if k != "val"} == {k: v for k, v in parent.items() if k != "val"}
    noval = tmp_path / "noval.yml"
    noval.write_text(yaml.safe_dump({k: v for k, v in opt.items() if k != "val"}))
    assert "val" not in T.parse_options(str(noval)) and T.parse_options(str(noval), u8=True)["val"] == {"u8_on_device": True}
    import inspect  # the command line carries the flag through to parse_options
    assert '"--u8"' in inspect.getsource(T.main) and "u8=args.u8" in inspect.getsource(T.main)
