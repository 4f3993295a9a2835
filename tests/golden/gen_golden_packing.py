"""Digests that pin every host-side weight packer (super_resolution_amd/packing.py, reached as `ops.pack_*`) to the bytes
the packers produced BEFORE they were rebuilt on one fragment helper: a packed weight is pure index gathering on CPU
tensors, so a refactor of the packers must reproduce it bit for bit.

Run on a checkout of the commit whose output is to be recorded (the fixture in git records the parent of the packing
refactor, 8c1ef91, whose packers still lived in ops.py):

    python tests/golden/gen_golden_packing.py <root of that checkout> [--time N]

Writes tests/golden/packing_digests.json (next to this file) = {"header": ..., "cases": {name: {"sha256": ..., scalars}}}.
--time N only prints the best-of-N wall time of the packing loop (no hashing) and writes nothing.

Weights come from integer arithmetic (`Wt`), never from an RNG, so every machine builds the same bytes.  A digest is the
sha256 over, for each non-None tensor attribute in order, str((shape, dtype)) followed by the tensor's contiguous raw bytes.
tests/test_packing_cpu.py loads this file by path and recomputes every case with the packers of its own tree.
"""
from __future__ import annotations

import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "packing_digests.json")
TENSORS = {"PackedFFN": ("w1f", "b1", "dww", "dwb", "w2f", "b2"), "PackedMlp": ("w1f", "b1", "w2f", "b2"), "PackedConv": ("w", "bias")}
SCALARS = ("nt", "n_slices", "kpad", "cin", "ksize", "nout", "chunks", "C", "hid", "ks", "frag")


def Wt(*shape, k=1):
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.int64) * 2654435761 * k) % 1021 - 510).float() / 256).reshape(shape)


def ffn_weights(C, h):
    return [Wt(2 * h, C), Wt(2 * h, k=3), Wt(2 * h, 1, 3, 3, k=5), Wt(2 * h, k=7), Wt(C, h, k=11), Wt(C, k=13)]


def pixel_shuffle_perm(o, r):
    """engine._pack_ps: packed row ij * cps + c  <-  original channel c * r^2 + ij."""
    cps, n = o // (r * r), torch.arange(o)
    return (n % cps) * (r * r) + n // cps


def pack_all(ops):
    """[(case name, packed object)] of every case, all on device 'cpu'."""
    BF16, F32 = ops.HAT_BF16, ops.HAT_F32
    out = []
    for C, h in ((144, 288), (180, 360), (24, 48)):
        out.append((f"ffn {C}", ops.pack_ffn(*ffn_weights(C, h), BF16, "cpu")))
    out.append(("ffn 24 f32", ops.pack_ffn(*ffn_weights(24, 48), F32, "cpu")))
    out.append(("ffn2", ops.pack_ffn2(*ffn_weights(144, 288), "cpu")))
    for C, h in ((144, 288), (180, 360)):
        out.append((f"ffn3 {C}", ops.pack_ffn3(*ffn_weights(C, h), Wt(C, k=17), Wt(C, k=19), "cpu")))
    out.append(("ocab_mlp", ops.pack_ocab_mlp(Wt(288, 144), Wt(288, k=3), Wt(144, 288, k=5), Wt(144, k=7), "cpu")))
    out.append(("ocab_qkv", ops.pack_ocab_qkv(Wt(144, 144), Wt(144, k=3), Wt(288, 144, k=5), None, 0.2, "cpu")))
    for o, i in ((144, 144), (288, 144), (360, 180), (180, 360), (64, 16)):
        out.append((f"linear {o}x{i}", ops.pack_linear_weight(Wt(o, i), Wt(o, k=3), BF16, "cpu")))
    out.append(("linear 3x3", ops.pack_linear_weight(Wt(144, 6, 3, 3), Wt(144, k=3), BF16, "cpu")))
    out.append(("squeeze 144", ops.pack_cab_squeeze(Wt(6, 144, 3, 3), Wt(6, k=3), "cpu")))
    out.append(("squeeze 64", ops.pack_cab_squeeze(Wt(3, 64, 3, 3), Wt(3, k=3), "cpu")))
    out.append(("w2f", ops.pack_cab_w2f(Wt(144, 6, 3, 3), "cpu")))
    out.append(("conv 144", ops.pack_conv_weight(Wt(144, 144, 3, 3), Wt(144), BF16, "cpu")))
    out.append(("conv nt1", ops.pack_conv_weight(Wt(3, 64, 3, 3), Wt(3, k=3), BF16, "cpu")))                     # conv_last: one n-tile
    out.append(("conv nt4 f32 scaled", ops.pack_conv_weight(Wt(60, 20, k=5), None, F32, "cpu", scale=0.5, nt=4)))   # (O, I) weight, Cin padded
    out.append(("conv pixelshuffle", ops.pack_conv_weight(Wt(256, 64, 3, 3), Wt(256, k=3), BF16, "cpu", out_perm=pixel_shuffle_perm(256, 2))))
    return out


def describe(p):
    """{"sha256": digest of the packed tensors, + the scalar attributes the object has}."""
    kind = type(p).__name__
    tensors = list(p) if isinstance(p, tuple) else ([p] if isinstance(p, torch.Tensor) else [getattr(p, a) for a in TENSORS[kind]])
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            continue
        h.update(str((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    d = {"sha256": h.hexdigest()}
    for a in SCALARS:
        if kind in TENSORS and hasattr(p, a):
            d[a] = getattr(p, a)
    return d


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    ops = importlib.import_module("super_resolution_amd.ops")
    assert os.path.abspath(ops.__file__).startswith(root), ops.__file__
    if "--time" in sys.argv:
        best = float("inf")
        for _ in range(int(sys.argv[sys.argv.index("--time") + 1])):
            t0 = time.perf_counter()
            pack_all(ops)
            best = min(best, time.perf_counter() - t0)
        print(f"packing loop, no hashing: best {best * 1e3:.1f} ms")
        return
    commit = subprocess.run(["git", "-C", root, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip()
    cases = {name: describe(p) for name, p in pack_all(ops)}
    for name, d in cases.items():
        print(f"{name:22s} {d['sha256'][:12]}")
    header = ("sha256 digests of the packed weights as the packers in ops.py produced them at the parent of the packing refactor "
              f"(commit {commit or 'unknown'}), generated by tests/golden/gen_golden_packing.py from a checkout of that commit")
    with open(FIXTURE, "w") as f:
        json.dump({"header": header, "torch": torch.__version__.split("+")[0], "cases": cases}, f, indent=1)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
