"""hat_window_attention (include/hat_mi355x.h) on operands a test controls: an fp64 restatement of the (S)W-MSA core written by index
arithmetic in the kernel's frame of reference, deliberately wrong variants of it (SLIPS), and the seeded case builders that
test_wmsa_ref_cpu.py and test_gpu_wmsa.py share.

The restatement uses no torch.roll, no window partition and no sw_msa_mask, so it shares no code with oracle/hat_oracle.py;
test_wmsa_ref_cpu.py pins it to O.window_msa, and shows that every slip leaves the bf16 bars of helpers.check by a factor of two on
at least one case family — a kernel that carries the slip and is otherwise within the bar then still fails."""
import functools

import torch

from helpers import q as rq, rnd

SLIPS = ["mask_replaces", "mask_minus_inf", "mask_adds_twice", "bands_swapped", "roll_reversed", "bias_not_flipped", "bias_transposed",
         "head_slices_shifted", "no_wrap"]

SHIFTS = {16: (0, 4, 8, 12), 8: (0, 4)}                  # every shift hat_window_attention admits (a multiple of 4 below ws)
# (H, W, B) at ws 16: one window; one window row; one window column (every window is a last column); 12 windows (no multiple of the
# 8 the fast kernel deals at a time); exactly 8; 9 (a second deal of which 7 workgroups per head return early).  ws 8: the same
# window counts at half the size.
GEOMS = {16: [(16, 16, 1), (16, 48, 1), (48, 16, 1), (32, 48, 2), (64, 32, 1), (48, 48, 1)]}
GEOMS[8] = [(h // 2, w // 2, b) for h, w, b in GEOMS[16]]
MAIN = {16: (32, 48, 2), 8: (16, 24, 2)}                 # the frame of every row that does not run the whole product

# (dtype, ws, C, heads, full): the kernel each row reaches follows from the dispatch of hat_window_attention (csrc/hat_attn.hip; DESIGN.md
# §4.0e): bf16 with ws 16 and head size 24 (rows / pointers aligned as the tests' default layout has them) or 30 takes
# ocab_attn_fast_kernel<D, 16, true>; everything else ocab_attn_kernel<T, ws^2 / 16, ., true>.  full: geometry x shift product.
CASES = [
    ("f32", 16, 48, 2, True),      # generic f32, d 24
    ("f32", 16, 180, 6, False),    # generic f32, d 30
    ("f32", 16, 64, 2, False),     # generic f32, d 32: no zero padding anywhere (dk8 == d)
    ("f32", 16, 32, 2, False),     # generic f32, d 16
    ("f32", 16, 20, 2, False),     # generic f32, d 10: dk8 = 16 > d, dv = 10
    ("f32", 16, 12, 2, False),     # generic f32, d 6
    ("f32", 16, 4, 2, False),      # generic f32, d 2
    ("bf16", 16, 144, 6, True),    # fast24
    ("bf16", 16, 180, 6, True),    # fast30
    ("bf16", 16, 64, 2, False),    # generic bf16 <16 tiles, chunks of 8>, d 32
    ("bf16", 16, 32, 2, False),    # generic bf16, d 16
    ("bf16", 16, 20, 2, False),    # generic bf16, d 10
    ("f32", 8, 48, 6, False),      # generic f32 <4 tiles, one chunk>, d 8
    ("f32", 8, 24, 2, False),      # generic f32, d 12
    ("f32", 8, 64, 2, False),      # generic f32, d 32
    ("bf16", 8, 48, 6, False),     # generic bf16, d 8
    ("bf16", 8, 24, 2, False),     # generic bf16, d 12
    ("bf16", 8, 64, 2, False),     # generic bf16, d 32
]
ROW_ID = lambda r: f"{r[0]}-ws{r[1]}-C{r[2]}-d{r[2] // r[3]}"
# one row per kernel family, for the tests that are about layout and addressing rather than head sizes
FAMILIES = [("bf16", 16, 144, 6), ("bf16", 16, 180, 6), ("bf16", 16, 64, 2), ("f32", 16, 48, 2), ("f32", 8, 48, 6), ("bf16", 8, 24, 2)]


def core_matrix():
    """(row, geom, shift) of test_core_matches_fp64."""
    out = []
    for row in CASES:
        ws = row[1]
        if row[4]:
            out += [(row, g, s) for g in GEOMS[ws] for s in SHIFTS[ws]]
        else:
            out += [(row, MAIN[ws], s) for s in sorted({0, 4, SHIFTS[ws][-1]})]
    return out


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def wmsa_core(q, k, v, table, ws: int, heads: int, shift: int, slip=None, probs=False):
    """hat_window_attention in fp64.  q (already scaled), k, v: (B,H,W,C); table ((2ws-1)^2, heads) as the reference holds it, looked
    up by relative_position_index = (qr - kr + ws-1) * (2ws-1) + (qc - kc + ws-1).  Window (wy, wx) position (r, c) is position
    (wy ws + r, wx ws + c) of the shifted frame = pixel ((wy ws + r + shift) % H, (wx ws + c + shift) % W); a frame coordinate t
    of an axis of n pixels is in band 0 below n - ws, 1 below n - shift, else 2 (swinir_arch.py:262-280), and a (query, key) pair
    whose row bands or column bands differ gets -100 ADDED once.  Output at the un-shifted pixel.  slip: one of SLIPS, a mutant.
    probs: also return the softmax weights (B, nWy, nWx, heads, ws^2, ws^2)."""
    assert slip is None or slip in SLIPS, slip
    B, H, W, C = q.shape
    d, n, nwy, nwx = C // heads, ws * ws, H // ws, W // ws
    q, k, v, table = q.double(), k.double(), v.double(), table.double()
    pos = torch.arange(n)
    r, c = pos // ws, pos % ws
    fy = torch.arange(nwy)[:, None] * ws + r[None, :]           # (nWy, n): frame row of every window position
    fx = torch.arange(nwx)[:, None] * ws + c[None, :]           # (nWx, n)
    sh = -shift if slip == "roll_reversed" else shift
    py, px = ((fy + sh) % H)[:, None, :], ((fx + sh) % W)[None, :, :]

    def windows(x):                                             # (B,H,W,C) -> (B, nWy, nWx, heads, n, d)
        return x[:, py, px].reshape(B, nwy, nwx, n, heads, d).permute(0, 1, 2, 4, 3, 5)

    qw, kw, vw = windows(q), windows(k), windows(v)
    if slip == "no_wrap":                                       # keys past the frame edge read as zeros
        live = ((fy + shift < H)[:, None, :] & (fx + shift < W)[None, :, :]).to(q.dtype)[None, :, :, None, :, None]
        kw, vw = kw * live, vw * live
    if slip == "head_slices_shifted":
        vw = vw.roll(-1, dims=3)
    logit = qw @ kw.transpose(-2, -1)                           # (B, nWy, nWx, heads, n query, n key)

    dr, dc = r[:, None] - r[None, :], c[:, None] - c[None, :]   # query - key
    if slip == "bias_not_flipped":
        dr, dc = -dr, -dc
    if slip == "bias_transposed":
        dr, dc = dc, dr
    rpi = (dr + ws - 1) * (2 * ws - 1) + (dc + ws - 1)
    logit = logit + table[rpi.reshape(-1)].reshape(n, n, heads).permute(2, 0, 1)

    edge = ws - shift if slip == "bands_swapped" else shift
    band = lambda t, size: (t >= size - ws).long() + (t >= size - edge).long()
    rb, cb = band(fy, H), band(fx, W)
    rdiff = (rb[:, :, None] != rb[:, None, :])[:, None]         # (nWy, 1, n, n)
    cdiff = (cb[:, :, None] != cb[:, None, :])[None, :]         # (1, nWx, n, n)
    diff = (rdiff | cdiff)[None, :, :, None]
    if slip == "mask_replaces":
        logit = torch.where(diff, torch.full_like(logit, -100.0), logit)
    elif slip == "mask_minus_inf":
        logit = torch.where(diff, torch.full_like(logit, float("-inf")), logit)
    elif slip == "mask_adds_twice":
        logit = logit - 100.0 * (rdiff.long() + cdiff.long())[None, :, :, None]
    else:
        logit = logit - 100.0 * diff
    p = torch.softmax(logit, dim=-1)
    o = (p @ vw).permute(0, 1, 2, 4, 3, 5).reshape(B, nwy, nwx, n, C)
    out = torch.empty(B, H, W, C, dtype=torch.float64)
    out[:, ((fy + sh) % H)[:, None, :], ((fx + sh) % W)[None, :, :]] = o
    return (out, p) if probs else out


def pixel(geom, ws, shift, wy, wx, r, c):
    """Pixel of position (r, c) of window (wy, wx) on the frame shifted by `shift`."""
    return (wy * ws + r + shift) % geom[0], (wx * ws + c + shift) % geom[1]


class Case:
    """Operands of one call (rounded to the storage type) and its fp64 reference, computed once and never modified."""

    def __init__(self, name, dtype, ws, heads, shift, geom, q, k, v, table, **extra):
        self.name, self.dtype, self.ws, self.heads, self.shift, self.geom = name, dtype, ws, heads, shift, geom
        self.q, self.k, self.v, self.table = q, k, v, table
        self.C = q.shape[-1]
        self.__dict__.update(extra)
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = self.core()
        return self._ref

    def core(self, slip=None, probs=False):
        return wmsa_core(self.q, self.k, self.v, self.table, self.ws, self.heads, self.shift, slip, probs)

    @property
    def bias_flip(self):
        """[heads][(2ws-1)^2] as the kernel indexes it (by key - query)."""
        return self.table.flip(0).t().contiguous()


def _qkv(tag, C, heads, geom, dtype):
    H, W, B = geom
    d = C // heads
    return (rq(rnd(tag + "q", (B, H, W, C)) * d ** -0.5, dtype), rnd(tag + "k", (B, H, W, C)), rq(rnd(tag + "v", (B, H, W, C)), dtype))


@functools.lru_cache(maxsize=None)
def random_case(C, heads, ws, geom, shift=0, dtype="f32"):
    """q, k, v ~ N(0, 1), q times d^-0.5; table std 2.0 (the module tests' is 0.5), so that the bias decides the softmax."""
    tag = f"wm{C}.{heads}.{ws}.{geom}"
    qv, k, v = _qkv(tag, C, heads, geom, dtype)
    return Case(f"random {dtype} C{C} ws{ws} {geom} shift {shift}", dtype, ws, heads, shift, geom, qv, rq(k, dtype), v,
                rnd(tag + "t", ((2 * ws - 1) ** 2, heads), std=2.0))


@functools.lru_cache(maxsize=None)
def mask_case(ws, shift, over, C=48, heads=2, geom=None, dtype="f32"):
    """Table zero; q and k zero but for channel 0 of every head at one (query, key) pair per kind of last window — last row (row
    bands differ), last column (column bands differ), corner (both differ) — where q = 13 (over) or 6 and k = 10: q.k = 130 leaves
    logit 30 after the mask is ADDED and the masked key takes essentially all the weight, q.k = 60 leaves -40 and it takes none.
    Every other logit of the frame is 0 or -100.  v ~ N(0, 1).  pairs: (wy, wx, query position, key position)."""
    geom = geom or MAIN[ws]
    H, W, B = geom
    nwy, nwx, d = H // ws, W // ws, C // heads
    assert shift > 0 and nwy >= 2 and nwx >= 2
    qv, k = torch.zeros(B, H, W, C), torch.zeros(B, H, W, C)
    kinds = [(nwy - 1, 0, (0, 1), (ws - 1, 2)), (0, nwx - 1, (1, 0), (2, ws - 1)), (nwy - 1, nwx - 1, (0, 0), (ws - 1, ws - 1))]
    pairs = []
    for wy, wx, qp, kp in kinds:
        qy, qx = pixel(geom, ws, shift, wy, wx, *qp)
        ky, kx = pixel(geom, ws, shift, wy, wx, *kp)
        qv[:, qy, qx, ::d] = 13.0 if over else 6.0
        k[:, ky, kx, ::d] = 10.0
        pairs.append((wy, wx, qp[0] * ws + qp[1], kp[0] * ws + kp[1]))
    v = rq(rnd(f"wmm{C}.{ws}.{geom}v", (B, H, W, C)), dtype)
    return Case(f"mask {dtype} C{C} ws{ws} shift {shift} over={over}", dtype, ws, heads, shift, geom, qv, k, v,
                torch.zeros((2 * ws - 1) ** 2, heads), pairs=pairs)


def selector_offsets(ws):
    return [(0, 0), (ws - 1, ws - 1), (-(ws - 1), ws - 1), (3, -5)]


@functools.lru_cache(maxsize=None)
def selector_case(ws, shift, dy, dx, C=48, heads=2, geom=None, dtype="f32"):
    """q = 0 and the table is +40 at the one entry a key at window offset (dy, dx) from its query is looked up at, 0 elsewhere; channels 0 and 1
    of every head of v hold the pixel's row / ws and column / ws (exact in bf16), the rest N(0, 1).  A query whose (r + dy, c + dx)
    lies in its window and in its band returns that key's v row (the others weigh e^-40 each); every other query returns the mean
    over its band."""
    geom = geom or MAIN[ws]
    H, W, B = geom
    d = C // heads
    tag = f"wms{C}.{ws}.{geom}"
    table = torch.zeros((2 * ws - 1) ** 2, heads)
    table[(-dy + ws - 1) * (2 * ws - 1) + (-dx + ws - 1)] = 40.0          # relative_position_index of query - key = (-dy, -dx)
    v = rnd(tag + "v", (B, H, W, C))
    v[..., 0::d] = (torch.arange(H, dtype=torch.float32) / ws)[None, :, None, None]
    v[..., 1::d] = (torch.arange(W, dtype=torch.float32) / ws)[None, None, :, None]
    return Case(f"selector {dtype} C{C} ws{ws} shift {shift} offset ({dy}, {dx})", dtype, ws, heads, shift, geom, torch.zeros(B, H, W, C),
                rq(rnd(tag + "k", (B, H, W, C)), dtype), rq(v, dtype), table, offset=(dy, dx))


SPIKES = ["last", "first", "masked"]


@functools.lru_cache(maxsize=None)
def spike_case(ws, shift, where, C=48, heads=2, geom=None, dtype="f32"):
    """random_case with k of one key of every window times 40 (as test_ocab_attention_softmax_spike): `last` the bottom-right key
    (last chunk: the rescale of everything before it), `first` the top-left key (first chunk: later chunks underflow against it),
    `masked` the first key row of the other band of a last-row window (window row ws - shift; row 0 without a shift)."""
    geom = geom or MAIN[ws]
    H, W, B = geom
    tag = f"wm{C}.{heads}.{ws}.{geom}"
    qv, k, v = _qkv(tag, C, heads, geom, dtype)
    r, c = {"last": (ws - 1, ws - 1), "first": (0, 0), "masked": ((ws - shift) % ws, ws // 2)}[where]
    for wy in range(H // ws):
        for wx in range(W // ws):
            y, x = pixel(geom, ws, shift, wy, wx, r, c)
            k[:, y, x] *= 40.0
    return Case(f"spike {dtype} C{C} ws{ws} shift {shift} {where}", dtype, ws, heads, shift, geom, qv, rq(k, dtype), v,
                rnd(tag + "t", ((2 * ws - 1) ** 2, heads), std=2.0), spike=(r, c))
