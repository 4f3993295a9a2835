"""Upscale a YUV4MPEG2 file on the device: 4:2:0 frames up, 4:2:0 frames down, no colour conversion on the host.

    python -m super_resolution_amd.video -opt options/test/HAT-S_SRx4.yml -i in.y4m -o out.y4m [--matrix bt709] [--full-range]
                                         [--out-depth 10] [--out-chroma 444] [--self-ensemble [N]]
                                         [--chroma-loc auto|center|left|topleft] [--out-chroma-loc ...]
    python -m super_resolution_amd.video --lte-model esc-lte.pth --size 1080 1920 -i 720p.y4m -o 1080p.y4m [the flags above]

y4m.Reader -> frames.upscale_frames(pixfmt='i420') -> y4m.Writer.  W and H of the header are multiplied by the network's
scale; every other header token (frame rate, interlacing, aspect, colour space, X comments) is copied.  Decoding and
encoding compressed video is somebody else's job: `ffmpeg -i in.mp4 -pix_fmt yuv420p in.y4m` and back.
10-, 12- and 16-bit streams (C420p10 / C420p12 / C420p16, `-pix_fmt yuv420p10le -strict -1`) are read as they are: the input
depth comes from the header; --out-depth sets the output's (default: the input's) and with it the output's C token, so
`--out-depth 10` on an 8-bit file writes the network's result with ten bits.  No transfer function is applied.
4:2:2, 4:4:4 and grey streams (C422 / C444 / Cmono and their deep forms) are read as they are; --out-chroma 420|422|444|mono
sets the output's subsampling (default: the input's) and with it the C token: `--out-chroma 444` on a 4:2:0 file keeps all of the
network's chroma.
--chroma-loc auto|center|left|topleft names the chroma siting of the input (yuv.py, "Chroma siting"); the default, center, treats
every stream as this tool always did.  auto takes it from the header (y4m.siting_of: C420mpeg2 is left, C420paldv top-left; a
4:2:2 header cannot say, so ask for left).  --out-chroma-loc sets the output's (default: the input's), and the written header
says what was written.
--self-ensemble [N] runs every frame through the geometric self-ensemble of N = 2, 4 or 8 (the default) members.
--lte-model ckpt.pth, in place of -opt, loads the arbitrary-scale network (ESCLTE.from_checkpoint, the reference's esc_arb checkpoint)
and needs --size H W or --scale S: the output stream has exactly that size (int(h S), int(w S) with --scale), even where the output's
chroma is subsampled; W and H of the header are set to it and every other token is copied (y4m.sized_header).  --self-ensemble does
not go with it.
Packed 4:2:2 (uyvy, yuy2, y210, v210: yuv.py, "Packed 4:2:2") does not fit a Y4M file, so either side can be a HEADERLESS file instead
(rawvideo.py; `ffmpeg -f rawvideo -pix_fmt uyvy422 | yuyv422 | y210le | v210`): --pixfmt F --raw-size H W [--raw-depth N] says what the
input holds, --out-pixfmt F makes the output headerless.  A side is Y4M when its flag is absent, so `--out-pixfmt v210` on a .y4m file
writes v210, and `--pixfmt uyvy --raw-size 1080 1920` with a .y4m output writes a C422 stream (whose header then names W, H and C
only).  uyvy / yuy2 are 8-bit, v210 is 10-bit, y210 takes --raw-depth / --out-depth 10 (the default), 12 or 16.

    python -m super_resolution_amd.video -opt options/test/HAT-S_SRx4.yml --pixfmt uyvy --raw-size 720 1280 -i in.uyvy --out-pixfmt uyvy \
                                         -o out.uyvy --chroma-loc left
"""
from __future__ import annotations

import argparse

from . import y4m


def upscale_file(net, src: str, dst: str, *, matrix: str = "bt601", full_range: bool = False, out_depth=None, ensemble: int = 1,
                 out_chroma=None, chroma_loc: str = "center", out_chroma_loc=None, size=None, scale=None, pixfmt=None, raw_size=None,
                 raw_depth=None, out_pixfmt=None) -> dict:
    """Every frame of the .y4m file `src` through `net` into `dst`; returns {'frames', 'in', 'out'} (sizes as (w, h)), and for
    streams that are not 8-bit on both sides also 'depth' and 'out_depth'; with ensemble 2 / 4 / 8 (the self-ensemble of every
    frame, frames.upscale_frames) also 'ensemble'; for streams that are not 4:2:0 on both sides also 'chroma' and 'out_chroma'
    (out_chroma '420' / '422' / '444' / 'mono'; default: the input's).  chroma_loc 'auto' / 'center' / 'left' / 'topleft': the
    input's chroma siting ('auto': y4m.siting_of the header); out_chroma_loc: the output's (default: the input's).  Unless both
    are 'center' — then the header is copied as always — the result also holds 'chroma_loc' and 'out_chroma_loc' and the output
    header names the output's siting (y4m.with_siting).
    size=(h, w) or scale=: `net` is an arbitrary-scale network (ESCLTE; frames.upscale_frames' size= / scale=) and the output stream
    has that size.
    pixfmt (yuv.PACKED_FORMATS) with raw_size=(h, w) and raw_depth: `src` is a headerless file of packed 4:2:2 frames (rawvideo.Reader);
    out_pixfmt: `dst` is one (rawvideo.Writer).  A side without its keyword is Y4M: upscale_packed_file."""
    from . import frames
    from .ops import ensemble_members
    ensemble = ensemble_members(ensemble)
    if pixfmt is not None or out_pixfmt is not None:
        return upscale_packed_file(net, src, dst, matrix=matrix, full_range=full_range, out_depth=out_depth, ensemble=ensemble,
                                   out_chroma=out_chroma, chroma_loc=chroma_loc, out_chroma_loc=out_chroma_loc, size=size, scale=scale,
                                   pixfmt=pixfmt, raw_size=raw_size, raw_depth=raw_depth, out_pixfmt=out_pixfmt)
    n = 0
    with y4m.Reader(src, chroma=True) as rd:
        depth = rd.depth
        out_depth = depth if out_depth is None else out_depth
        chroma = y4m.chroma(rd.header)
        out_chroma = chroma if out_chroma is None else out_chroma
        if size is None and scale is None:
            sized, akw = y4m.scaled_header(rd.header, net.upscale), {}
        else:
            if (size is None) == (scale is None):
                raise ValueError("upscale_file takes exactly one of size=(h, w) and scale=, or neither")
            oh, ow = (int(rd.h * scale), int(rd.w * scale)) if size is None else (int(size[0]), int(size[1]))
            sized, akw = y4m.sized_header(rd.header, ow, oh), {"size": (oh, ow)}
        hdr = y4m.with_chroma(y4m.with_depth(sized, out_depth), out_chroma)
        siting, out_siting = resolve_chroma_loc(rd.header, chroma_loc, out_chroma_loc)
        skw = {} if (siting, out_siting) == ("center", "center") else {"siting": siting, "out_siting": out_siting}
        if skw:
            hdr = y4m.with_siting(hdr, out_siting)
        kw = {} if depth == 8 and out_depth == 8 else {"depth": depth, "out_depth": out_depth}
        if ensemble > 1:
            kw["ensemble"] = ensemble
        info = {} if chroma == "420" and out_chroma == "420" else {"chroma": chroma, "out_chroma": out_chroma}
        fkw = {"out_pixfmt": y4m.CHROMAS[out_chroma]} if info else {}
        with y4m.Writer(dst, hdr, chroma=True) as wr:
            for out in frames.upscale_frames(net, rd, pixfmt=rd.fmt, matrix=matrix, full_range=full_range, **kw, **fkw, **skw, **akw):
                wr.write(out)
                n += 1
    loc = {"chroma_loc": siting, "out_chroma_loc": out_siting} if skw else {}
    return dict({"frames": n, "in": (rd.w, rd.h), "out": (hdr["W"], hdr["H"])}, **kw, **info, **loc)


def check_raw_args(pixfmt, raw_size, raw_depth, out_pixfmt, out_depth):
    """The headerless sides' arguments, refused in words (RuntimeError): -> (depth of a headerless input or None, depth of a headerless
    output or None: the caller's default)."""
    from . import yuv
    if pixfmt is None:
        if raw_size is not None or raw_depth is not None:
            raise RuntimeError("--raw-size and --raw-depth describe a headerless input: they need --pixfmt")
        depth = None
    else:
        if raw_size is None:
            raise RuntimeError(f"a headerless {pixfmt} file does not say its size: --pixfmt needs --raw-size H W")
        depth = yuv.packed_container(pixfmt, raw_depth)[1]
        yuv.packed_shape(raw_size[0], raw_size[1], pixfmt)
    if out_pixfmt is not None and out_depth is not None:
        yuv.packed_container(out_pixfmt, out_depth)
    return depth


def upscale_packed_file(net, src: str, dst: str, *, matrix="bt601", full_range=False, out_depth=None, ensemble=1, out_chroma=None,
                        chroma_loc="center", out_chroma_loc=None, size=None, scale=None, pixfmt=None, raw_size=None, raw_depth=None,
                        out_pixfmt=None) -> dict:
    """upscale_file with a headerless packed 4:2:2 file (rawvideo.py) on the input side (pixfmt, raw_size, raw_depth), the output side
    (out_pixfmt) or both; the other side, if any, is Y4M.  Returns {'frames', 'in', 'out', 'pixfmt', 'out_pixfmt', 'depth', 'out_depth'}."""
    from . import frames, rawvideo, yuv
    depth = check_raw_args(pixfmt, raw_size, raw_depth, out_pixfmt, out_depth)
    if out_pixfmt is not None and out_chroma is not None:
        raise RuntimeError("--out-chroma names the subsampling of a Y4M output: a packed output is 4:2:2")
    if (size is not None) and (scale is not None):
        raise ValueError("upscale_file takes exactly one of size=(h, w) and scale=, or neither")
    n = 0
    rd = rawvideo.Reader(src, pixfmt, raw_size[0], raw_size[1], depth) if pixfmt is not None else y4m.Reader(src, chroma=True)
    with rd:
        in_fmt, depth = rd.fmt, rd.depth
        header = {"W": rd.w, "H": rd.h, "X": []} if pixfmt is not None else rd.header
        if size is None and scale is None:
            oh, ow, akw = rd.h * net.upscale, rd.w * net.upscale, {}
        else:
            oh, ow = (int(rd.h * scale), int(rd.w * scale)) if size is None else (int(size[0]), int(size[1]))
            akw = {"size": (oh, ow)}
        siting, out_siting = resolve_chroma_loc(header, chroma_loc, out_chroma_loc)
        if out_pixfmt is not None:
            if out_depth is None:   # the input's where the layout takes it, else the layout's own
                out_depth = depth if out_pixfmt == "y210" and depth in (10, 12, 16) else yuv.packed_container(out_pixfmt)[1]
            wr, out_fmt = rawvideo.Writer(dst, out_pixfmt, oh, ow, out_depth), out_pixfmt
        else:
            out_depth = depth if out_depth is None else out_depth
            out_chroma = ("422" if pixfmt is not None else y4m.chroma(header)) if out_chroma is None else out_chroma
            hdr = y4m.with_chroma(y4m.with_depth(y4m.sized_header(header, ow, oh), out_depth), out_chroma)
            if (siting, out_siting) != ("center", "center"):
                hdr = y4m.with_siting(hdr, out_siting)
            wr, out_fmt = y4m.Writer(dst, hdr, chroma=True), y4m.CHROMAS[out_chroma]
        kw = {"ensemble": ensemble} if ensemble > 1 else {}
        wkw = {"width": rd.w} if pixfmt is not None else {}
        with wr:
            for out in frames.upscale_frames(net, rd, pixfmt=in_fmt, out_pixfmt=out_fmt, matrix=matrix, full_range=full_range, depth=depth,
                                             out_depth=out_depth, siting=siting, out_siting=out_siting, **kw, **wkw, **akw):
                wr.write(out)
                n += 1
    return {"frames": n, "in": (rd.w, rd.h), "out": (ow, oh), "pixfmt": in_fmt, "out_pixfmt": out_fmt, "depth": depth, "out_depth": out_depth}


CHROMA_LOCS = ("auto", "center", "left", "topleft")


def resolve_chroma_loc(header: dict, chroma_loc: str = "center", out_chroma_loc=None):
    """(siting, out_siting) of a run on a stream with this header: 'auto' is y4m.siting_of(header), None the input's."""
    for v in (chroma_loc, out_chroma_loc):
        if v is not None and v not in CHROMA_LOCS:
            raise RuntimeError(f"unknown chroma location {v!r}: one of {CHROMA_LOCS}")
    siting = y4m.siting_of(header) if chroma_loc == "auto" else chroma_loc
    out_siting = siting if out_chroma_loc is None else y4m.siting_of(header) if out_chroma_loc == "auto" else out_chroma_loc
    return siting, out_siting


class _Parser(argparse.ArgumentParser):
    """The flags that depend on each other are checked where the others are: parse_args exits on them as on a bad choice."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if (ns.opt is None) == (ns.lte_model is None):
            self.error("one of -opt (a fixed-scale network) and --lte-model (the arbitrary-scale network) is required")
        if ns.lte_model is not None:
            if (ns.size is None) == (ns.scale is None):
                self.error("--lte-model needs exactly one of --size H W and --scale S")
            if ns.self_ensemble is not None:
                self.error("--self-ensemble is not built for --lte-model")
            if ns.scale is not None and not ns.scale > 0:
                self.error("--scale must be positive")
            if ns.size is not None and min(ns.size) < 1:
                self.error("--size must be positive")
        elif ns.size is not None or ns.scale is not None:
            self.error("--size and --scale belong to --lte-model: a network loaded with -opt has a fixed scale")
        try:
            check_raw_args(ns.pixfmt, ns.raw_size, ns.raw_depth, ns.out_pixfmt, ns.out_depth)
        except RuntimeError as e:
            self.error(str(e))
        return ns


def parser() -> argparse.ArgumentParser:
    ap = _Parser(description="upscale a YUV4MPEG2 (.y4m) file of 4:2:0 video (8, 10, 12 or 16 bits) on the device")
    ap.add_argument("-opt", default=None, help="test YAML (network_g, path.pretrain_network_g ...), as for super_resolution_amd.test")
    ap.add_argument("--lte-model", default=None, metavar="CKPT",
                    help="in place of -opt: a checkpoint of the arbitrary-scale ESC-LTE (the reference's esc_arb format); needs --size or --scale")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"), help="with --lte-model: the output size")
    ap.add_argument("--scale", type=float, default=None, metavar="S", help="with --lte-model: the output is int(h S) x int(w S)")
    ap.add_argument("--compute-dtype", default="bf16", choices=["bf16", "fp32"], help="with --lte-model: the compute dtype (default: bf16)")
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709", "bt2020nc"],
                    help="YCbCr matrix of the stream (default: bt601, the reference's)")
    ap.add_argument("--out-depth", type=int, default=None, choices=[8, 10, 12, 16],
                    help="bits per sample of the output stream (default: the input's, which the header names)")
    ap.add_argument("--out-chroma", default=None, choices=["420", "422", "444", "mono"],
                    help="chroma subsampling of the output stream (default: the input's, which the header names)")
    ap.add_argument("--chroma-loc", default="center", choices=list(CHROMA_LOCS),
                    help="chroma siting of the input: center (default: JPEG / MPEG-1, every stream as before), left (MPEG-2, H.264, HEVC, "
                         "AV1; all 4:2:2), topleft (BT.2020), or auto: what the header says (C420mpeg2 left, C420paldv topleft)")
    ap.add_argument("--out-chroma-loc", default=None, choices=list(CHROMA_LOCS),
                    help="chroma siting of the output stream (default: the input's); the output header names it")
    ap.add_argument("--pixfmt", default=None, choices=["uyvy", "yuy2", "y210", "v210"],
                    help="the input is a HEADERLESS file of packed 4:2:2 frames in this layout (needs --raw-size); absent: a .y4m file")
    ap.add_argument("--raw-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="with --pixfmt: the size of the input's frames")
    ap.add_argument("--raw-depth", type=int, default=None, choices=[8, 10, 12, 16],
                    help="with --pixfmt: bits per sample (uyvy / yuy2: 8; v210: 10; y210: 10, 12 or 16, default 10)")
    ap.add_argument("--out-pixfmt", default=None, choices=["uyvy", "yuy2", "y210", "v210"],
                    help="write a HEADERLESS file of packed 4:2:2 frames in this layout; absent: a .y4m file")
    ap.add_argument("--full-range", action="store_true", help="the stream is full range (0-255) instead of 16-235 / 16-240")
    ap.add_argument("--self-ensemble", nargs="?", type=int, const=8, default=None, choices=[2, 4, 8], metavar="N",
                    help="geometric self-ensemble of every frame over the first N = 2, 4 or 8 (default when N is left out) flips / transposes")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    if args.lte_model is not None:
        import torch
        from .archs.esc_lte_arch import ESCLTE
        net = ESCLTE.from_checkpoint(torch.load(args.lte_model, map_location="cpu", weights_only=True), compute_dtype=args.compute_dtype).to(args.device)
    else:
        from .models import HATModel
        from .test import parse_options
        model = HATModel(parse_options(args.opt), device=args.device)
        net = model.get_bare_model(model.net_g)
    info = upscale_file(net, args.input, args.output, matrix=args.matrix, full_range=args.full_range,
                        out_depth=args.out_depth, ensemble=args.self_ensemble or 1, out_chroma=args.out_chroma, chroma_loc=args.chroma_loc,
                        out_chroma_loc=args.out_chroma_loc, size=args.size, scale=args.scale, pixfmt=args.pixfmt, raw_size=args.raw_size,
                        raw_depth=args.raw_depth, out_pixfmt=args.out_pixfmt)
    print(info)
    return info


if __name__ == "__main__":
    main()
