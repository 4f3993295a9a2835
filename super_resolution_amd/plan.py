"""Forward plans: export one input shape's complete HAT forward for hosts without Python.

    python -m super_resolution_amd.plan -opt options/test/x.yml --shape 1 720 1280 -o net_720p.hatplan
    plan.export_plan(net, (1, 3, 720, 1280), "net_720p.hatplan")

The exporter runs ONE forward of the engine on the GPU with a recording proxy in front of the C ABI: every launch call
(`hat_conv`, `hat_hab_tail`, ...) is captured with its arguments, every device pointer in them is resolved to (buffer,
offset) against the tensors the engine owns (packed weights, per-shape workspace) plus the input and the output, and the
list is written with the weights' bytes to a file that `hat_plan_load` / `hat_plan_forward` (csrc/hat_plan.cpp,
include/hat_mi355x.h "Forward plans") replay from C.  Whatever kernel sequence the engine chooses for the model and shape
is what the plan contains; results are bit-identical to `net(x)`.  `record_plan` does the recording, `plan_bytes` the writing
(no torch, no GPU: it also builds files by hand); `hat_plan_load` checks a file in full before it allocates
(csrc/hat_plan_parse.h).

File format (little endian): "HATPLAN1", u32 version = HAT_ABI_VERSION, u32 n_buffers, u32 n_calls, u32 n_functions, i32 dims[8] =
{B, Cin, H, W, scale, Cout, dtype, 0}; buffers {u32 kind (0 const, 1 scratch, 2 input, 3 output), u32 0, u64 bytes,
[bytes padded to 8 if const]}; calls {u32 function id, u32 n_args, args {u32 tag, u32 0, payload}} with payloads
int: i64 | float: f64 | pointer: u32 buffer (0xFFFFFFFF = NULL), u32 0, u64 offset | struct / host array: u32 bytes,
u32 n_fixups, image padded to 8, fixups {u32 field offset, u32 buffer, u64 offset} | stream: nothing.
"""
from __future__ import annotations

import argparse
import bisect
import ctypes as C
import struct
import threading
from typing import List, Tuple

import torch

from . import _lib

# function ids = index in this list (csrc/hat_plan_parse.h HAT_PLAN_FUNCTIONS mirrors it)
FN_IDS = ["hat_conv", "hat_linear", "hat_conv3x3_small", "hat_cab_fold", "hat_aggr_cab", "hat_ffn", "hat_ffn2", "hat_hab_tail",
          "hat_layernorm", "hat_esc_weights", "hat_eca_scale", "hat_dwconv_gate", "hat_sgfn_gate", "hat_ocab_attention",
          "hat_window_attention", "hat_cab_squeeze", "hat_conv3x3_to_planes", "hat_add_f32", "hat_esc_conv13", "hat_ocab_keybias", "hat_ocab_attention_kb", "hat_ocab_mlp", "hat_ocab_qkv", "hat_hab_tail3", "hat_ocab_attention_log2", "hat_naf_half",
          "hat_naf_fold"]
ARG_INT, ARG_FLOAT, ARG_PTR, ARG_STRUCT, ARG_HOST, ARG_STREAM = range(6)
BUF_CONST, BUF_SCRATCH, BUF_INPUT, BUF_OUTPUT = range(4)
NULL_BUF = 0xFFFFFFFF
_EXPORT_LOCK = threading.Lock()


class _Recorder:
    """Stands in for the loaded library while one forward is recorded: forwards every call, keeps the launches."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []
        self._tid = threading.get_ident()    # only the exporting thread's launches belong to the plan

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in FN_IDS:
            return fn      # queries (tile counts, plans): not launches

        def call(*args):
            if threading.get_ident() == self._tid:   # (another thread's forward passes through unrecorded)
                self.calls.append((name, [_snapshot(a) for a in args]))
            return fn(*args)
        return call


def _snapshot(a):
    """Copy an argument at call time (descriptors are reused / mutated by the caller afterwards)."""
    obj = getattr(a, "_obj", None)           # ctypes.byref(struct)
    if isinstance(obj, C.Structure):
        return ("struct", type(obj), bytes(memoryview(obj)))
    if isinstance(a, C.Array):
        return ("host", bytes(memoryview(a)))
    return a


def _pointer_fields(stype, base=0) -> List[int]:
    out = []
    for name, ftype in stype._fields_:
        off = base + getattr(stype, name).offset
        if isinstance(ftype, type) and issubclass(ftype, C.Structure):
            out += _pointer_fields(ftype, off)
        elif ftype is C.c_void_p:
            out.append(off)
    return out


def _tensors_of(obj, seen, out):
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            out.append(obj)
        return
    if isinstance(obj, dict):
        for v in obj.values():
            _tensors_of(v, seen, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors_of(v, seen, out)
    elif hasattr(obj, "__dict__") or hasattr(obj, "__slots__"):
        for k in list(getattr(obj, "__dict__", {})) + list(getattr(obj, "__slots__", ())):
            if k not in ("_lock", "_s1"):
                _tensors_of(getattr(obj, k, None), seen, out)


def plan_bytes(dims, buffers, calls, offsets=None) -> bytes:
    """The file of a plan (format: this module's docstring) from plain values; touches neither torch nor the GPU.

    dims     the eight int32 {B, Cin, H, W, scale, Cout, dtype, 0}
    buffers  [(kind, nbytes, data)]: data = the bytes of a BUF_CONST buffer (written as they are, padded to 8), else None
    calls    [(name or function id, [argument ...])] with arguments ("int", v) | ("float", v) | ("ptr", buffer, offset) |
             ("struct", image, [(field offset, buffer, offset) ...]) | ("host", image) | ("stream",); NULL_BUF = a null pointer
    offsets  a dict to fill with where things went: "dims", "buffers" (each buffer's header: u32 kind, u32 0, u64 bytes),
             "calls" ([{"at": the call's header (u32 function id, u32 n_args), "args": each argument's header (u32 tag, u32 0;
             the payload follows at + 8)}]) and "end" — what a test patches a file by."""
    pad8 = lambda data: bytes(data) + b"\0" * ((8 - len(data) % 8) % 8)
    where = {"dims": 24, "buffers": [], "calls": []}
    out = bytearray()
    out += b"HATPLAN1" + struct.pack("<4I", _lib.ABI_VERSION, len(buffers), len(calls), len(FN_IDS))
    out += struct.pack("<8i", *dims)
    for kind, nbytes, data in buffers:
        where["buffers"].append(len(out))
        out += struct.pack("<IIQ", kind, 0, nbytes)
        if data is not None:
            out += pad8(data)
    for fn, args in calls:
        entry = {"at": len(out), "args": []}
        where["calls"].append(entry)
        out += struct.pack("<II", fn if isinstance(fn, int) else FN_IDS.index(fn), len(args))
        for a in args:
            entry["args"].append(len(out))
            if a[0] == "struct":
                _, image, fixes = a
                out += struct.pack("<IIII", ARG_STRUCT, 0, len(image), len(fixes)) + pad8(image)
                for off, bi, bo in fixes:
                    out += struct.pack("<IIQ", off, bi, bo)
            elif a[0] == "host":
                out += struct.pack("<IIII", ARG_HOST, 0, len(a[1]), 0) + pad8(a[1])
            elif a[0] == "stream":
                out += struct.pack("<II", ARG_STREAM, 0)
            elif a[0] == "ptr":
                out += struct.pack("<IIIIQ", ARG_PTR, 0, a[1], 0, a[2])
            elif a[0] == "float":
                out += struct.pack("<IId", ARG_FLOAT, 0, float(a[1]))
            elif a[0] == "int":
                out += struct.pack("<IIq", ARG_INT, 0, int(a[1]))
            else:
                raise ValueError(f"plan_bytes: unknown argument form {a[0]!r}")
    where["end"] = len(out)
    if offsets is not None:
        offsets.update(where)
    return bytes(out)


def record_plan(net, x_shape: Tuple[int, int, int, int]):
    """Run ONE forward of `net`'s engine for inputs of `x_shape` = (B, Cin, H, W) on the module's device behind the recorder and
    return what plan_bytes takes: (dims, buffers, calls), every device pointer resolved to (buffer, offset)."""
    eng = net.engine()
    dev = eng.dev
    if not hasattr(eng, "pe_norm"):
        raise NotImplementedError(f"a plan records HATEngine's call list: {type(net).__name__} cannot be exported yet (DESIGN.md §7)")
    if eng.pe_norm is None:
        raise NotImplementedError("patch_norm=False copies a tensor with a torch op, which a plan cannot record")
    B, Cin, H, W = x_shape
    x = torch.zeros(x_shape, dtype=torch.float32, device=dev)
    real = _lib.load()
    rec = _Recorder(real)
    with _EXPORT_LOCK:                         # one export at a time: the recorder stands in for the process-wide library handle
        _lib._lib = rec
        try:
            # a plan holds the unguarded entries: a C host has no guard; and the head as its three launches: the
            # function table's size is the file format, and hat_head_fused writes what they write, bit for bit
            with torch.no_grad(), eng.guard_mode("off"), eng.head_route(fused=False):
                y = eng.forward(x, one_stream=True)   # the plan replays on one stream: record the launches in that order
            torch.cuda.synchronize(dev)
        finally:
            _lib._lib = real
    ws = eng._workspace(B, H, W)
    consts, scratch = [], []
    _tensors_of({k: v for k, v in eng.__dict__.items() if k not in ("_ws_cache", "_guard")}, set(), consts)
    _tensors_of(ws, set(), scratch)

    # buffers = distinct storages; kind by where the tensor came from
    bufs, index = [], {}

    def add(t, kind):
        st = t.untyped_storage()
        key = st.data_ptr()
        if key in index:
            return
        index[key] = len(bufs)
        bufs.append({"kind": kind, "start": key, "nbytes": st.nbytes(), "storage": st, "tensor": t})

    add(x, BUF_INPUT)
    add(y, BUF_OUTPUT)
    for t in scratch:
        add(t, BUF_SCRATCH)
    for t in consts:
        add(t, BUF_CONST)
    starts = sorted((b["start"], i) for i, b in enumerate(bufs))
    keys = [s for s, _ in starts]

    def resolve(p):
        if not p:
            return NULL_BUF, 0
        k = bisect.bisect_right(keys, p) - 1
        if k >= 0:
            b = bufs[starts[k][1]]
            if p < b["start"] + max(b["nbytes"], 1):
                return starts[k][1], p - b["start"]
        raise RuntimeError(f"plan export: device pointer {p:#x} does not belong to the engine's weights, its workspace, the input "
                           f"or the output (a temporary allocated inside forward?)")

    buffers = []
    for b in bufs:
        data = None
        if b["kind"] == BUF_CONST:
            raw = torch.empty(b["nbytes"], dtype=torch.uint8, device="cpu")
            raw.copy_(torch.tensor([], dtype=torch.uint8, device=dev).set_(b["storage"], 0, (b["nbytes"],)))
            data = raw.numpy().tobytes()
        buffers.append((b["kind"], b["nbytes"], data))
    calls = []
    for name, args in rec.calls:
        sig = _lib.SIGNATURES[name][1]
        out = []
        for k, a in enumerate(args):
            if isinstance(a, tuple) and a[0] == "struct":
                _, stype, image = a
                out.append(("struct", image, [(off,) + resolve(struct.unpack_from("<Q", image, off)[0]) for off in _pointer_fields(stype)]))
            elif isinstance(a, tuple) and a[0] == "host":
                out.append(("host", a[1]))
            elif k == len(args) - 1:                     # every launch entry point ends with the stream
                out.append(("stream",))
            elif sig[k] is C.c_void_p:
                out.append(("ptr",) + resolve(a))
            elif sig[k] is C.c_float:
                out.append(("float", a))
            else:
                out.append(("int", a))
        calls.append((name, out))
    return (B, Cin, H, W, eng.scale, y.shape[1], eng.dtype, 0), buffers, calls


def export_plan(net, x_shape: Tuple[int, int, int, int], path: str) -> dict:
    """Record `net`'s forward for inputs of `x_shape` = (B, Cin, H, W) on the module's device and write the plan file."""
    dims, buffers, calls = record_plan(net, x_shape)
    out = plan_bytes(dims, buffers, calls)
    with open(path, "wb") as f:
        f.write(out)
    return {"path": path, "launches": len(calls), "buffers": len(buffers), "file_bytes": len(out),
            "const_bytes": sum(n for kind, n, _ in buffers if kind == BUF_CONST),
            "scratch_bytes": sum(n for kind, n, _ in buffers if kind == BUF_SCRATCH),
            "functions": sorted({name for name, _ in calls})}


class Plan:
    """ctypes view of hat_plan_load / hat_plan_forward / hat_plan_free — what a C host does (used by the tests)."""

    def __init__(self, path: str):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._lib.hat_plan_load(path.encode(), C.byref(self._h)), f"hat_plan_load({path})")
        dims = (C.c_int32 * 8)()
        n, nb = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.hat_plan_info(self._h, dims, C.byref(n), C.byref(nb)), "hat_plan_info")
        self.dims, self.launches, self.device_bytes = list(dims), n.value, nb.value

    def forward(self, x: torch.Tensor, y: torch.Tensor, stream: int = 0):
        _lib.check(self._lib.hat_plan_forward(self._h, x.data_ptr(), y.data_ptr(), stream), "hat_plan_forward")

    def forward_u8(self, src: torch.Tensor, dst: torch.Tensor, *, bgr: bool = False, stream: int = 0):
        """hat_plan_forward_u8: src (B,h,w,3) uint8 device frames with h <= H, w <= W of the plan (reflect-padded to (H, W) on
        the device) -> dst (B,s*h,s*w,3) uint8.  Rows may be pitched; samples must lie h (s*h) rows apart.  The first call
        allocates the plan's fp32 staging buffers."""
        for t, rows in ((src, src.shape[1]), (dst, dst.shape[1])):
            if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.stride(3) != 1 or t.stride(2) != 3 \
                    or (t.shape[0] > 1 and t.stride(0) != rows * t.stride(1)):
                raise RuntimeError("forward_u8 needs (B,h,w,3) uint8 device tensors with interleaved pixels and samples h rows apart")
        s, (h, w) = self.dims[4], src.shape[1:3]
        if src.shape[0] != self.dims[0] or tuple(dst.shape) != (self.dims[0], s * h, s * w, 3):
            raise RuntimeError(f"forward_u8: src {tuple(src.shape)} / dst {tuple(dst.shape)} do not match a plan of batch {self.dims[0]}, scale {s}")
        _lib.check(self._lib.hat_plan_forward_u8(self._h, src.data_ptr(), src.stride(1), h, w, dst.data_ptr(), dst.stride(1), int(bgr), stream),
                   "hat_plan_forward_u8")

    def _yuv_args(self, what, src, dst, size, shape, matrix, full_range, depth, out_depth):
        """What the YCbCr forwards start with: (h, w) = size(src.shape) of the source frames, the refusal of a dst that is not
        shape(s h, s w) frames of the plan's batch, and the two colour matrices of the depths as the C side takes them."""
        from . import ops, yuv
        to_rgb, from_rgb = yuv.csc(matrix, full_range, depth)[0], yuv.csc(matrix, full_range, out_depth)[1]
        h, w = size(src.shape)
        s = self.dims[4]
        if src.shape[0] != self.dims[0] or tuple(dst.shape) != (self.dims[0],) + shape(s * h, s * w):
            raise RuntimeError(f"{what}: src {tuple(src.shape)} / dst {tuple(dst.shape)} do not match a plan of batch {self.dims[0]}, scale {s}")
        return h, w, ops._f12(to_rgb), ops._f12(from_rgb)

    def forward_yuv420(self, src: torch.Tensor, dst: torch.Tensor, *, fmt: str = "nv12", matrix: str = "bt601", full_range: bool = False,
                       depth: int = 8, out_depth=None, msb=None, stream: int = 0, siting: str = "center", out_siting=None):
        """hat_plan_forward_yuv420: src (B,3h/2,w) uint8 device frames in the layout `fmt` with h <= H, w <= W of the plan
        (reflect-padded to (H, W) on the device) -> dst (B,3sh/2,sw) uint8 in the same layout.  The first byte-path call
        allocates the plan's fp32 staging buffers.  depth / out_depth / msb as HAT.forward_yuv420 takes them (uint16 tensors on a
        deep side): hat_plan_forward_yuv420_deep.  siting / out_siting other than 'center': forward_yuv's route
        (hat_plan_forward_yuv_sited) for the same frames."""
        from . import ops, yuv
        out_siting = yuv.check_siting(siting) if out_siting is None else yuv.check_siting(out_siting)
        if (siting, out_siting) != ("center", "center"):
            yuv.check_fmt(fmt), yuv.frame_size(src.shape)
            return self.forward_yuv(src, dst, fmt=fmt, out_fmt=fmt, matrix=matrix, full_range=full_range, depth=depth, out_depth=out_depth,
                                    msb=msb, out_msb=msb, stream=stream, siting=siting, out_siting=out_siting)
        out_depth = depth if out_depth is None else out_depth
        h, w, to_rgb, from_rgb = self._yuv_args("forward_yuv420", src, dst, yuv.frame_size, yuv.frame_shape, matrix, full_range, depth, out_depth)
        sb = ops._yuv_block(*ops.yuv420_views(src, fmt), "forward_yuv420")
        db = ops._yuv_block(*ops.yuv420_views(dst, fmt), "forward_yuv420")
        if depth == 8 and out_depth == 8:
            if src.dtype != torch.uint8 or dst.dtype != torch.uint8:
                raise TypeError(f"forward_yuv420: 8-bit frames are uint8 tensors, got {src.dtype} / {dst.dtype}")
            _lib.check(self._lib.hat_plan_forward_yuv420(self._h, *sb, h, w, *db, to_rgb, from_rgb, stream), "hat_plan_forward_yuv420")
            return
        for t, d in ((src, depth), (dst, out_depth)):
            if t.dtype != (torch.uint8 if d == 8 else torch.uint16):
                raise TypeError(f"forward_yuv420: depth {d} needs a {'uint8' if d == 8 else 'uint16'} tensor, got {t.dtype}")
        sm, dm = int(bool(yuv.container(depth, fmt, msb)[3])), int(bool(yuv.container(out_depth, fmt, msb)[3]))
        _lib.check(self._lib.hat_plan_forward_yuv420_deep(self._h, *sb, depth, sm, h, w, *db, out_depth, dm, to_rgb, from_rgb, stream),
                   "hat_plan_forward_yuv420_deep")

    def forward_yuv(self, src: torch.Tensor, dst: torch.Tensor, *, fmt: str, out_fmt=None, matrix: str = "bt601", full_range: bool = False,
                    depth: int = 8, out_depth=None, msb=None, out_msb=None, stream: int = 0, siting: str = "center", out_siting=None, width=None):
        """hat_plan_forward_yuv: src (B,rows,w) device frames in any layout `fmt` of yuv.LAYOUTS with h <= H, w <= W of the plan ->
        dst, the frames of the s-times larger image in the layout `out_fmt` (default: fmt).  Keywords as HAT.forward_yuv takes them;
        a siting or out_siting other than 'center' goes through hat_plan_forward_yuv_sited, and a fmt or out_fmt of
        yuv.PACKED_FORMATS (width= for 'v210') through hat_plan_forward_packed422."""
        from . import ops, yuv
        out_siting = yuv.check_siting(siting) if out_siting is None else yuv.check_siting(out_siting)
        out_fmt = fmt if out_fmt is None else out_fmt
        out_depth = depth if out_depth is None else out_depth
        a = ops.FrameSide(fmt, depth=depth, msb=msb, siting=siting)
        b = ops.FrameSide(out_fmt, depth=out_depth, msb=out_msb, siting=out_siting)
        h, w, to_rgb, from_rgb = self._yuv_args("forward_yuv", src, dst, lambda shape: a.size(shape, width), b.shape, matrix, full_range, depth,
                                                out_depth)

        def surface(side, t, wd):   # (the packed surface, the planar one, what keeps their pointers alive)
            if side.packed:
                if not side.rows_packed(t):
                    raise RuntimeError(f"forward_yuv needs {side.fmt} frames with packed rows, got strides {t.stride()}")
                return ops.packed_surface(t, side.fmt, width=wd, depth=side.depth, msb=side.msb, what="forward_yuv")[0], None, t
            v = side.views(t)
            return None, ops.yuv_surface(*v, sub=side.sub, depth=side.depth, msb=side.msb, what="forward_yuv"), v

        sp, ss, _keep_s = surface(a, src, w)
        dp, ds, _keep_d = surface(b, dst, self.dims[4] * w)
        ref = lambda x: None if x is None else C.byref(x)
        if a.packed or b.packed:
            _lib.check(self._lib.hat_plan_forward_packed422(self._h, ref(sp), ref(ss), yuv.SITINGS.index(siting), ref(dp), ref(ds),
                                                            yuv.SITINGS.index(out_siting), h, w, to_rgb, from_rgb, stream),
                       "hat_plan_forward_packed422")
            return
        if (siting, out_siting) != ("center", "center"):
            _lib.check(self._lib.hat_plan_forward_yuv_sited(self._h, C.byref(ss), yuv.SITINGS.index(siting), C.byref(ds),
                                                            yuv.SITINGS.index(out_siting), h, w, to_rgb, from_rgb, stream),
                       "hat_plan_forward_yuv_sited")
            return
        _lib.check(self._lib.hat_plan_forward_yuv(self._h, C.byref(ss), C.byref(ds), h, w, to_rgb, from_rgb, stream), "hat_plan_forward_yuv")

    def close(self):
        if self._h:
            self._lib.hat_plan_free(self._h)
            self._h = C.c_void_p()

    __del__ = close


def main(argv=None):
    ap = argparse.ArgumentParser(description="export a forward plan for hat_plan_load / hat_plan_forward")
    ap.add_argument("-opt", required=True, help="test YAML (network_g, path.pretrain_network_g ...), as for super_resolution_amd.test")
    ap.add_argument("--shape", type=int, nargs=3, metavar=("B", "H", "W"), required=True)
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from .models import HATModel
    from .test import parse_options
    opt = parse_options(args.opt)
    model = HATModel(opt, device=args.device)
    B, H, W = args.shape
    info = export_plan(model.net_g, (B, opt["network_g"].get("in_chans", 3), H, W), args.out)
    print(info)
    return info


if __name__ == "__main__":
    main()
