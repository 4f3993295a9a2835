"""Exact-lattice cases of hat_vgg_conv (tests/lattice.py's method): operands on the dyadic lattice and slopes that are powers of two
make the layer's result the one exactly representable fp32 number, so the kernel must equal the fp64 reference rounded once to T,
bit for bit.  Host only: test_gpu_srvgg.py launches these cases, test_srvgg_cpu.py checks their domain conditions."""
import torch

import lattice as L

# distinct powers of two from 2^-3 to 2^1 with both signs, plus 0: eleven values, dealt round-robin to the 64 channels
SLOPE_VALUES = [0.0] + [sg * 2.0 ** e for e in range(-3, 2) for sg in (1.0, -1.0)]
GEOMS = [(1, 1, 1), (1, 16, 16), (1, 19, 35), (2, 33, 40), (1, 1, 70), (1, 70, 1)]   # (B, H, W)
MODES = ["rows", "frame"]
UNIT = 0.125                                                                          # the result's lattice step: 2^-3


def slopes() -> torch.Tensor:
    return torch.tensor([SLOPE_VALUES[(5 * c + 3) % len(SLOPE_VALUES)] for c in range(64)], dtype=torch.float64)


def trips(tiles: int, wgs: int):
    """Trips of every workgroup of a slice under hat_vgg_conv's schedule: workgroup i takes the tiles i, i + wgs, ..."""
    return [-(-(tiles - i) // wgs) for i in range(min(wgs, tiles))]


def two_trip_geom(tiles_of):
    """The smallest frame (fewest pixels, B = 1) at which some workgroup takes two trips and another one.  tiles_of(B, H, W) ->
    (tiles, wgs, slices), the library's query.  The schedule grows wgs with the tile count up to its cap, so the first frame with
    tiles > wgs is a single row of tiles one longer than the cap."""
    w = 1
    while True:
        tiles, wgs, _ = tiles_of(1, 1, w)
        t = trips(tiles, wgs)
        if max(t) == 2 and min(t) == 1:
            return (1, 1, w)
        assert max(t) == 1 and w < 1 << 16
        w += 16


def vgg_case(geom, mode: str, dtype: str) -> L.Case:
    """x (B,H,W,cin) on the lattice (cin = 3 as planes for mode "frame", 64 as rows), w (64,cin,3,3), bias, slope; ref = the layer in
    fp64."""
    B, H, W = geom
    cin, st = (3 if mode == "frame" else 64), L.STORE[dtype]
    key = f"vgg.{mode}.{geom}"
    c = L.Case(geom=geom, mode=mode, dtype=dtype)
    c.x = L.acts(key + ".x", (B, H, W, cin))
    c.w = L.weights(key + ".w", (64, cin, 3, 3))
    c.bias = L.draw(key + ".b", (64,), 8)
    c.slope = slopes()
    s = L.conv64(c.x, c.w, c.bias)
    c.ref = torch.where(s >= 0, s, c.slope * s)
    absum = L.conv_abs(c.x, c.w, c.bias) * 2.0      # |slope| <= 2
    L.assert_exact_domain(f"{key}[{dtype}]", stored=[("x", c.x, st), ("x as fp32", c.x, torch.float32), ("w", c.w, st), ("bias", c.bias, torch.float32),
                                                    ("slope", c.slope, torch.float32)],
                          absum=absum, unit=UNIT, addends=[c.bias, s, c.ref])
    assert len(set(c.slope.tolist())) == len(SLOPE_VALUES)
    if s.numel() >= 4096:   # the negative side, where the slopes act, is there
        assert float((s < 0).double().mean()) > 0.2
    return c
