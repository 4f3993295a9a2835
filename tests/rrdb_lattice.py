"""Exact-lattice cases of hat_rdb_conv (tests/lattice.py's method): small-integer operands and slope / beta1 / beta2 that are powers of
two make a dense-block conv's result the one exactly representable fp32 number, so the kernel must equal the fp64 restatement
rounded once to T, bit for bit, and its fp32 stream output must equal it unrounded.  Host only: test_gpu_rrdb.py launches these
cases, test_rrdb_cpu.py checks their domain conditions."""
import torch

import lattice as L
from srvgg_lattice import trips, two_trip_geom  # noqa: F401  (the schedule is hat_vgg_conv's rule)

CINS = (64, 96, 128, 160, 192)
FORMS = {64: ["act"], 96: ["act"], 128: ["act"], 160: ["act"], 192: ["r1", "r1r2"]}
GEOMS = [(1, 1, 1), (1, 16, 16), (1, 19, 35), (2, 33, 40), (1, 1, 70), (1, 70, 1)]   # (B, H, W)
POW2 = [sg * 2.0 ** e for e in range(-3, 2) for sg in (1.0, -1.0)]                   # +-2^-3 .. +-2^1: ten values
LD = 200                                                                             # dense rows of 192 channels and 8 pad columns
UNIT = 2.0 ** -6                                                                     # the result's lattice step: beta2 beta1 at 2^-3 each


def params(cin: int, gi: int):
    """(slope, beta1, beta2) of a case: every (cin, geometry) takes another triple, all ten values are used over the table."""
    i = CINS.index(cin) + 3 * gi
    return POW2[i % 10], POW2[(i + 3) % 10], POW2[(i + 7) % 10]


def rdb_case(geom, cin: int, form: str) -> L.Case:
    """x (B,H,W,cin), w (cout,cin,3,3), bias on the integer lattice; r1 / r2 (B,H,W,64) on quarters; ref = the layer in fp64."""
    B, H, W = geom
    gi = GEOMS.index(geom) if geom in GEOMS else len(GEOMS)
    cout, key = (64 if cin == 192 else 32), f"rdb.{cin}.{form}.{geom}"
    c = L.Case(geom=geom, cin=cin, cout=cout, form=form)
    c.slope, c.beta1, c.beta2 = params(cin, gi)
    c.x = L.acts(key + ".x", (B, H, W, cin))
    c.w = L.weights(key + ".w", (cout, cin, 3, 3), density=0.25)
    c.bias = L.draw(key + ".b", (cout,), 8)
    s = L.conv64(c.x, c.w, c.bias)
    absum = L.conv_abs(c.x, c.w, c.bias)
    stored = [("x", c.x, torch.bfloat16), ("w", c.w, torch.bfloat16), ("bias", c.bias, torch.float32)]
    stored += [(n, torch.tensor(v), torch.float32) for n, v in (("slope", c.slope), ("beta1", c.beta1), ("beta2", c.beta2))]
    c.r1 = c.r2 = None
    if form == "act":
        c.ref = torch.where(s >= 0, s, c.slope * s)
        absum, addends = absum * 2.0, [c.bias, s, c.ref]
    else:
        c.r1 = L.draw(key + ".r1", (B, H, W, 64), 64, 2)
        c.ref = c.beta1 * s + c.r1
        absum, addends = absum * abs(c.beta1) + c.r1.abs(), [c.bias, c.beta1 * s, c.r1, c.ref]
        stored += [("r1", c.r1, torch.float32), ("r1 as T (hat_conv's r2)", c.r1, torch.bfloat16)]
        if form == "r1r2":
            c.r2 = L.draw(key + ".r2", (B, H, W, 64), 64, 2)
            c.ref = c.beta2 * c.ref + c.r2
            absum = absum * abs(c.beta2) + c.r2.abs()
            addends += [c.r2, c.ref]
            stored.append(("r2", c.r2, torch.float32))
    L.assert_exact_domain(key, stored=stored, absum=absum, unit=UNIT, addends=addends)
    if form == "act" and s.numel() >= 4096:   # the negative side, where the slope acts, is there
        assert float((s < 0).double().mean()) > 0.2
    return c
