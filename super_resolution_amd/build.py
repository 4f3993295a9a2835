"""Build libhat_mi355x.so (gfx950 code objects + the C ABI) in-tree with hipcc.

    python -m super_resolution_amd.build [--force]

hipcc cross-compiles for gfx950 without a GPU.  The library is written next to this file so it
travels with the source tree to the GPU box; it is git-ignored.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libhat_mi355x.so")
SOURCES = ["hat_conv.hip", "hat_conv64r.hip", "hat_attn.hip", "hat_misc.hip", "hat_ffn.hip", "hat_ffn2.hip", "hat_tail3.hip", "hat_tail3l.hip", "hat_pw.hip", "hat_mlp.hip", "hat_cabsq.hip", "hat_esc13.hip", "hat_upfold.hip", "hat_u8.hip", "hat_yuv.hip", "hat_packed422.hip", "hat_resize.hip", "hat_pil_resize.hip", "hat_metrics.hip", "hat_dihedral.hip", "hat_niqe.hip", "hat_naf.hip", "hat_esc.hip", "hat_escreal.hip", "hat_escrealm.hip", "hat_escfp.hip", "hat_lte.hip", "hat_esc_sink.hip", "hat_vgg.hip", "hat_rrdb.hip", "hat_head.hip", "hat_plan.cpp"]
HEADERS = [os.path.join(CSRC, "hat_common.h"), os.path.join(CSRC, "hat_yuv_check.h"), os.path.join(CSRC, "hat_packed_check.h"), os.path.join(CSRC, "hat_yuv_sample.h"), os.path.join(CSRC, "hat_frame_sink.h"), os.path.join(CSRC, "hat_esc_ffn.h"), os.path.join(CSRC, "hat_gated_ffn.h"), os.path.join(CSRC, "hat_conv3_tile.h"), os.path.join(CSRC, "hat_plan_parse.h"), os.path.join(os.path.dirname(HERE), "include", "hat_mi355x.h")]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    hipcc = _hipcc()
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        objs.append(o)
        if force or _stale(o, [s] + HEADERS):
            jobs.append([hipcc, *FLAGS, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
