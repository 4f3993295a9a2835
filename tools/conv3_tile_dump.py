"""tools/conv3_tile_dump.py — raw output bytes of the three resident-weight 3x3 convs (csrc/hat_conv3_tile.h) on seeded, normally
distributed inputs, one file per case, for a byte comparison of two builds of the library (profiles/conv3_tile_share_isa.txt):

    HAT_MI355X_LIB=<the other build's library> python tools/conv3_tile_dump.py <dir A>      (a fresh process per side)
    python tools/conv3_tile_dump.py <dir B> && for f in <dir A>/*; do cmp $f <dir B>/$(basename $f); done

Cases: hat_vgg_conv rows and frame x bf16 and fp32; hat_rdb_conv at its five cin, convs 1-4 in place (out == x, out_off == cin), conv 5
with r1, with r1 and r2, with neither, in place and into a second buffer as the engine runs it; hat_conv on the resident route as 64 ->
64 with LeakyReLU (1 slice) and 64 -> 256 with PixelShuffle 2 (4 slices).  Each at a small ragged frame with B = 2 and at the smallest
frame whose tile loop takes a second trip.  Every output buffer starts as the byte 0xA5, so a stray store shows."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 41
SMALL = (2, 33, 40)


def main():
    import torch
    from srvgg_lattice import trips, two_trip_geom
    from super_resolution_amd import ops, synth
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    total = 0

    def filled(shape, tdt):
        n = 1
        for s in shape:
            n *= s
        return torch.full((n * torch.empty((), dtype=tdt).element_size(),), 0xA5, dtype=torch.uint8, device=dev).view(tdt).reshape(shape)

    def normal(key, shape, tdt, std=1.0):
        return synth.normal(SEED, key, shape, std=std).to(dev).to(tdt).contiguous()

    def dump(name, *tensors):
        nonlocal total
        torch.cuda.synchronize()
        raw = b"".join(t.contiguous().view(torch.uint8).cpu().numpy().tobytes() for t in tensors)
        with open(os.path.join(outdir, name + ".bin"), "wb") as f:
            f.write(raw)
        total += len(raw)
        print(f"{name}: {len(raw)} bytes", flush=True)

    # ---- hat_vgg_conv ----
    for dname, dt in (("bf16", ops.HAT_BF16), ("f32", ops.HAT_F32)):
        tdt = ops.TORCH_DTYPE[dt]
        big = two_trip_geom(lambda B, H, W: ops.vgg_conv_tiles(B, H, W, dt))
        for mode, cin in (("rows", 64), ("frame", 3)):
            pv = ops.pack_vgg_conv(synth.normal(SEED, f"vw{cin}", (64, cin, 3, 3), std=(9 * cin) ** -0.5), synth.normal(SEED, "vb", (64,), std=0.1),
                                   synth.uniform(SEED, "vs", (64,)) - 0.3, dt, dev)
            for B, H, W in (SMALL, big):
                x = normal(f"vx{mode}", (B, 3, H, W), torch.float32) if cin == 3 else normal(f"vx{mode}", (B, H, W, 64), tdt)
                out = filled((B, H, W, 64), tdt)
                ops.vgg_conv(pv, x, out, B=B, H=H, W=W, dtype=dt)
                dump(f"vgg_{mode}_{dname}_{B}x{H}x{W}", out)

    # ---- hat_rdb_conv ----
    dt, tdt = ops.HAT_BF16, torch.bfloat16
    for cin in ops.RDB_CIN:
        cout = 64 if cin == 192 else 32
        pr = ops.pack_rdb_conv(synth.normal(SEED, f"rw{cin}", (cout, cin, 3, 3), std=(9 * cin) ** -0.5), synth.normal(SEED, f"rb{cin}", (cout,), std=0.1), dt, dev)
        big = two_trip_geom(lambda B, H, W: ops.rdb_conv_tiles(B, H, W, cin))
        for B, H, W in (SMALL, big):
            geo, tag = dict(B=B, H=H, W=W, dtype=dt), f"{B}x{H}x{W}"
            LD = cin + cout

            def rows():   # cin channels of data, the output slot behind them filled
                d = filled((B, H * W, LD), tdt)
                d[:, :, :cin] = normal(f"rx{cin}", (B, H * W, cin), tdt, std=0.5)
                return d

            if cin < 192:
                d = rows()
                ops.rdb_conv(pr, d, d, **geo, ldx=LD, ldo=LD, out_off=cin, slope=0.2)
                dump(f"rdb_{cin}_inplace_{tag}", d)
                continue
            r1, r2 = normal("rr1", (B, H * W, 64), torch.float32), normal("rr2", (B, H * W, 64), torch.float32)
            for res, kw in (("r1", dict(r1=r1)), ("r1r2", dict(r1=r1, r2=r2)), ("nores", {})):
                d, s_out = rows(), filled((B, H * W, 64), torch.float32)
                ops.rdb_conv(pr, d, d, **geo, ldx=LD, ldo=LD, out_off=cin, beta1=0.2, beta2=0.2, s_out=s_out, **kw)
                dump(f"rdb_192_{res}_inplace_{tag}", d, s_out)
            d, dn, s_out = rows(), filled((B, H * W, LD), tdt), filled((B, H * W, 64), torch.float32)
            ops.rdb_conv(pr, d, dn, **geo, ldx=LD, ldo=LD, out_off=0, beta1=0.2, beta2=0.2, r1=r1, r2=r2, s_out=s_out)
            dump(f"rdb_192_r1r2_engine_{tag}", dn, s_out)

    # ---- hat_conv -> conv64r_kernel ----
    for r in (0, 2):
        cout, nsl = (64 * r * r if r else 64), (r * r if r else 1)
        perm = None
        if r:
            n = torch.arange(cout)
            perm = (n % 64) * (r * r) + n // 64
        pw = ops.pack_conv_weight(synth.normal(SEED, f"cw{r}", (cout, 64, 3, 3), std=576 ** -0.5), synth.normal(SEED, f"cb{r}", (cout,), std=0.1), dt, dev, out_perm=perm)
        nwps = 8 * (32 // nsl)                                   # conv3_groups at its cap
        for B, H, W in ((2, 19, 21), (1, 1, 16 * nwps + 1)):     # the second: nwps + 1 tiles, one workgroup takes two trips
            assert (B, H, W) == (2, 19, 21) or sorted(set(trips(nwps + 1, nwps))) == [1, 2]
            x = normal(f"cx{r}", (B, H * W, 64), tdt)
            if r:
                out = filled((B, H * r * W * r, 64), tdt)
                ops.conv(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=64, ldo=64, out_mode=ops.O_PIXSHUF_T, ps_r=r)
            else:
                out = filled((B, H * W, 64), tdt)
                ops.conv(pw, x, out, B=B, H=H, W=W, dtype=dt, ldx=64, ldo=64, act=2)
            dump(f"conv64r_{'ps%d' % r if r else 'lrelu'}_{B}x{H}x{W}", out)
    print(f"total: {total} bytes", flush=True)


if __name__ == "__main__":
    main()
