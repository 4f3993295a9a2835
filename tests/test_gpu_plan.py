"""Forward plans (include/hat_mi355x.h "Forward plans"; SURVEY §8b's whole-network entry point): the launch list the
Python engine produces for one shape, exported to a file and replayed through hat_plan_load / hat_plan_forward — the
three calls a host without Python makes — must reproduce `net(x)` bit for bit, for a fresh input, in both precisions and
for every kernel sequence the engine has: fused (HAT-S), unfused (C = 24), embed_dim 180, `ape`, HATX plain / focus / live.
Every entry point a plan can hold is replayed by some case here (test_every_entry_point_is_replayed), and hat_plan_load
refuses changed copies of a real plan without touching the device (tests/test_plan_parse_cpu.py has every rule, on the host)."""
import ctypes as C
import os
import struct
from unittest import mock

import pytest
import torch

from helpers import META, W_SEED, X_SEED
from super_resolution_amd import synth

pytestmark = pytest.mark.gpu

# (arch, golden config, dtype, input shape): frames of one to six windows
CASES = {"hats_bf16": ("HAT", "hats_1g_x4", "bf16", (1, 3, 32, 48)), "hats_f32_B2": ("HAT", "hats_1g_x4", "f32", (2, 3, 16, 32)),
         "tiny_ocabesc": ("HAT", "tiny_ocabesc_x2", "bf16", (1, 3, 16, 24)), "hatx": ("HATX", "hatx_tiny_plain_x2", "f32", (1, 3, 16, 24)),
         "ape": ("HAT", "tiny_identity_ape_x2", "f32", (1, 3, 16, 16)),          # hat_add_f32 as the engine emits it (ape holds img_size^2 positions)
         "hat180_f32": ("HAT", "hat_1g_x2", "f32", (1, 3, 16, 16)),              # embed_dim 180: hat_eca_scale + unfused CAB convs, hat_ffn, tail3l
         "hat180_bf16": ("HAT", "hat_1g_x2", "bf16", (1, 3, 16, 32)),
         "hatx_focus": ("HATX", "hatx_tiny_focus_x2", "f32", (1, 3, 8, 16)),     # hat_ocab_keybias / hat_ocab_attention_kb
         "hatx_live": ("HATX", "hatx_live_x2", "bf16", (1, 3, 8, 16)),           # hat_sgfn_gate at the live widths
         "hats_bf16_B2": ("HAT", "hats_1g_x4", "bf16", (2, 3, 16, 16)),
         # the engine's older kernel sequences (engine.Options: same arithmetic, chosen when the engine is built)
         "hats_no_tail": ("HAT", "hats_1g_x4", "bf16", (1, 3, 16, 16), {"HAT_NO_HAB_TAIL": "1"}),    # hat_aggr_cab, then hat_ffn2
         "tiny_unfused_ffn": ("HAT", "tiny_x2", "f32", (1, 3, 8, 8), {"HAT_NO_FUSED_FFN": "1"})}     # fc1, hat_dwconv_gate, fc2
_FUNCTIONS = {}     # case id -> the entry points its plan calls (filled by whichever test exports the case first)


def _net(arch, name, dtype, dev, env=None):
    """The network with its engine built (under the switches of `env`, which the engine reads once, when it is built)."""
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    net = build_network(dict(type=arch, compute_dtype=dtype, **META["cfgs"][name])).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    net = net.to(dev)
    with mock.patch.dict(os.environ, env or {}):
        net.engine()
    return net


@pytest.mark.parametrize("case", list(CASES))
def test_plan_replay_is_bit_identical(case, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from super_resolution_amd import plan
    arch, name, dtype, shape = CASES[case][:4]
    dev = torch.device("cuda:0")
    net = _net(arch, name, dtype, dev, *CASES[case][4:])
    path = str(tmp_path / "net.hatplan")
    info = plan.export_plan(net, shape, path)
    _FUNCTIONS[case] = info["functions"]
    assert info["launches"] > 10 and info["const_bytes"] > 0
    x = synth.synth_input(X_SEED + 1, shape).to(dev)        # not the tensor the plan was recorded with
    ref = net(x).clone()
    p = plan.Plan(path)
    assert p.dims[:4] == list(shape) and p.launches == info["launches"]
    s = META["cfgs"][name]["upscale"]
    y = torch.full((shape[0], 3, shape[2] * s, shape[3] * s), 5.0, device=dev)
    p.forward(x, y, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    y2 = torch.zeros_like(y)                                  # a second forward on the same plan (workspace reuse)
    p.forward(x, y2, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y2, ref)
    p.close()


# Entry points of the function table that no engine path emits any more.  They stay in the table because the table's order is
# the file format (HAT_ABI_VERSION 2), and tests/test_plan_parse_cpu.py still checks their marshalling against the binding.
NOT_EMITTED = [
    # the second-generation fused tail (ffn2_kernel<aggr>): ops.hab_tail launches it for a pack_ffn2 FFN, but the engine's two
    # fused tails (_tail_fused144 / _tail_fused180) pass hb.ffn3, the hat_hab_tail3 packing, since Options.tail_v2 was removed
    "hat_hab_tail",
    # (S)W-MSA core: only archs/window_msa.WindowAttention calls it, a stand-alone module (this fork's HAB has no window
    # attention); HATEngine.forward, which is all a plan records, never does
    "hat_window_attention",
]


def test_every_entry_point_is_replayed(tmp_path):
    """The union of what the cases above and the NAF-stem network (tests/test_gpu_naf.py replays it) record is the whole function
    table but NOT_EMITTED: dispatch() has no call site that only a hand-built file reaches."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import naf_ref as R
    from super_resolution_amd import plan
    from super_resolution_amd.registry import build_network
    dev = torch.device("cuda:0")
    for case, (arch, name, dtype, shape, *env) in CASES.items():
        if case not in _FUNCTIONS:      # (run on its own: export what the replay test would have)
            _FUNCTIONS[case] = plan.export_plan(_net(arch, name, dtype, dev, *env), shape, str(tmp_path / "net.hatplan"))["functions"]
    naf = build_network(dict(type="HybridHATNAF", compute_dtype="f32", **R.net_kwargs(R.NAMES[32]))).eval()
    naf.load_state_dict(R.synth_sd(R.NAMES[32]), strict=True)
    seen = set(plan.export_plan(naf.to(dev), (1, 3, 16, 24), str(tmp_path / "naf.hatplan"))["functions"])
    for case, names in _FUNCTIONS.items():
        assert names == sorted(set(names)) and set(names) <= set(plan.FN_IDS), case
        seen |= set(names)
    assert set(NOT_EMITTED) <= set(plan.FN_IDS)
    missing, revived = set(plan.FN_IDS) - set(NOT_EMITTED) - seen, seen & set(NOT_EMITTED)
    assert not missing, f"no case replays {sorted(missing)}"
    assert not revived, f"{sorted(revived)} are emitted again: take them off NOT_EMITTED"


def test_plan_load_rejects_garbage(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from super_resolution_amd import plan
    bad = tmp_path / "bad.hatplan"
    bad.write_bytes(b"NOTAPLAN" + b"\0" * 64)
    with pytest.raises(RuntimeError):
        plan.Plan(str(bad))
    with pytest.raises(RuntimeError):
        plan.Plan(str(tmp_path / "missing.hatplan"))


@pytest.fixture(scope="module")
def recorded():
    """One real plan — tiny_x2, fp32, one window — as (dims, buffers, calls) and as bytes with the writer's offsets."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from super_resolution_amd import plan
    dims, buffers, calls = plan.record_plan(_net("HAT", "tiny_x2", "f32", torch.device("cuda:0")), (1, 3, 8, 8))
    where = {}
    return dims, buffers, calls, plan.plan_bytes(dims, buffers, calls, where), where


def _first(calls, pred):
    return next((i, k) for i, (name, args) in enumerate(calls) for k, a in enumerate(args) if pred(name, k, a))


def _short_struct(dims, buffers, calls, data, where, plan):
    i, k = _first(calls, lambda name, k, a: a[0] == "struct")
    calls = [(n, list(a)) for n, a in calls]
    calls[i][1][k] = ("struct", calls[i][1][k][1][:8], [])        # an 8-byte blob where the descriptor goes
    return plan.plan_bytes(dims, buffers, calls)


def _wrong_tag(dims, buffers, calls, data, where, plan):
    i, k = _first(calls, lambda name, k, a: a[0] == "ptr")
    calls = [(n, list(a)) for n, a in calls]
    calls[i][1][k] = ("int", 0)                                   # P() of it would be a null pointer
    return plan.plan_bytes(dims, buffers, calls)


def _int32_overflow(dims, buffers, calls, data, where, plan):
    from super_resolution_amd import _lib
    i, k = _first(calls, lambda name, k, a: a[0] == "int" and _lib.SIGNATURES[name][1][k] is C.c_int32)
    out = bytearray(data)
    struct.pack_into("<q", out, where["calls"][i]["args"][k] + 8, 2 ** 32 + int(calls[i][1][k][1]))     # the same low 32 bits
    return bytes(out)


def _zero_height(dims, buffers, calls, data, where, plan):
    out = bytearray(data)
    struct.pack_into("<i", out, where["dims"] + 8, 0)
    return bytes(out)


def _short_input(dims, buffers, calls, data, where, plan):
    i = next(i for i, b in enumerate(buffers) if b[0] == plan.BUF_INPUT)
    out = bytearray(data)
    struct.pack_into("<Q", out, where["buffers"][i] + 8, buffers[i][1] - 4)       # one float fewer than B*Cin*H*W
    return bytes(out)


def _cut_in_a_constant(dims, buffers, calls, data, where, plan):
    i = max(i for i, b in enumerate(buffers) if b[0] == plan.BUF_CONST and b[1] >= 16)
    return data[:where["buffers"][i] + 16 + 8]                   # the file ends 8 bytes into that buffer's data


def _trailing_byte(dims, buffers, calls, data, where, plan):
    return data + b"\0"


@pytest.mark.parametrize("change", [_short_struct, _wrong_tag, _int32_overflow, _zero_height, _short_input, _cut_in_a_constant, _trailing_byte],
                         ids=lambda f: f.__name__.strip("_"))
def test_plan_load_refuses_a_changed_plan(change, recorded, tmp_path):
    """hat_plan_load on copies of a real plan with one field changed.  Loading is all that happens: a refused file is parsed on
    the host and nothing is allocated or launched for it; no copy declares a larger buffer than the original, and none is ever
    given to a forward."""
    from super_resolution_amd import plan
    dims, buffers, calls, data, where = recorded
    bad = change(dims, buffers, calls, data, where, plan)
    assert bad != data
    path = tmp_path / "bad.hatplan"
    path.write_bytes(bad)
    with pytest.raises(RuntimeError, match="HAT_EINVAL"):
        plan.Plan(str(path))
    good = tmp_path / "good.hatplan"
    good.write_bytes(data)                   # the unchanged bytes load
    p = plan.Plan(str(good))
    assert p.dims == list(dims) and p.launches == len(calls)
    p.close()


def test_c_host_program_runs_a_plan(tmp_path):
    """The C example (no Python in the process that computes): export a plan here, then run examples/plan_forward.c built with
    gcc as a child process on it and check that it reports the output mean the Python engine gets for the same input."""
    import os
    import re
    import shutil
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    from super_resolution_amd import plan
    from super_resolution_amd.registry import build_network
    import super_resolution_amd.archs  # noqa: F401
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "plan_forward"
    r = subprocess.run(["gcc", os.path.join(root, "examples", "plan_forward.c"), "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-L" + os.path.join(root, "super_resolution_amd"), "-lhat_mi355x", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + os.path.join(root, "super_resolution_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    dev = torch.device("cuda:0")
    shape = (1, 3, 32, 32)
    net = build_network(dict(type="HAT", compute_dtype="bf16", **META["cfgs"]["hats_1g_x4"])).eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), W_SEED), strict=True)
    net = net.to(dev)
    path = str(tmp_path / "net.hatplan")
    plan.export_plan(net, shape, path)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    x = ((torch.arange(n, dtype=torch.int64) * 2654435761) % 1000).to(torch.float32).div(1000.0).reshape(shape)   # the example's image (64-bit product)
    ref = float(net(x.to(dev)).double().mean())
    r = subprocess.run([str(exe), path, "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"mean of the output (-?[0-9.]+)", r.stdout)
    assert m, r.stdout
    assert abs(float(m.group(1)) - ref) <= 2e-5, (r.stdout, ref)
