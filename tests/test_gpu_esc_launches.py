"""The launches of one forward of every ESC-family network against tests/golden/esc_launches.json, which was recorded before the
engines were taken apart into stem, residual and head parts (tests/golden/gen_golden_esc_launches.py): the same kernels, in the
same instantiations, in the same order.  What the launches compute is the other ESC tests' subject."""
from __future__ import annotations

import json
import os

import pytest
import torch

import esc_launches as L

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "esc_launches.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_the_fixture_has_the_cases():
    assert set(GOLDEN) == set(L.CASES)
    for name, (typ, kw, frame) in L.CASES.items():
        g = GOLDEN[name]
        assert (g["type"], g["kw"], tuple(g["frame"])) == (typ, kw, tuple(frame)), name


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("name", list(L.CASES))
def test_launches_are_the_recorded_ones(name, dtype):
    got, outs, _ = L.run_case(name, dtype, torch.device("cuda:0"))
    want = GOLDEN[name][dtype]
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{name} [{dtype}]: {len(got)} launches against {len(want)} recorded; the first difference is launch {first}: " \
                        f"{got[first:first + 1]} against {want[first:first + 1]}"
