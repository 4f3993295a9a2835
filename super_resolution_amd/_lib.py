"""ctypes binding of libhat_mi355x.so (the C ABI declared in include/hat_mi355x.h).

There is NO fallback: if the library is missing, cannot be loaded, or an entry point is absent,
every use raises.  Build it with `python -m super_resolution_amd.build` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HAT_MI355X_LIB") or os.path.join(_HERE, "libhat_mi355x.so")  # env override: A/B builds

ABI_VERSION = 2   # == HAT_ABI_VERSION of include/hat_mi355x.h: bump both whenever a descriptor or packing changes
HAT_F32, HAT_BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_LRELU, ACT_LRELU02 = 0, 1, 2, 3   # LRELU: slope 0.01; LRELU02: slope 0.2, hat_conv only
X_NHWC_T, X_NHWC_F32, X_NCHW_F32_MEAN = 0, 1, 2
O_NHWC_T, O_NHWC_F32, O_PIXSHUF_T, O_NCHW_F32, O_FOLD2_NCHW_F32 = 0, 1, 2, 3, 4
METRICS_Y, METRICS_BGR, METRICS_PSNR, METRICS_SSIM = 1, 2, 4, 8   # flags of hat_u8_metrics

_ERRORS = {-1: "HAT_EINVAL (bad argument)", -2: "HAT_ELDS (tile does not fit in 160 KiB LDS)",
           -3: "HAT_EUNSUPPORTED (shape not instantiated)"}


class HatConvDesc(C.Structure):
    """Mirror of `struct HatConvDesc` (include/hat_mi355x.h) — field order and types must match."""
    _fields_ = [
        ("x", C.c_void_p), ("x0", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("out", C.c_void_p), ("r1", C.c_void_p), ("r2", C.c_void_p), ("r2scale", C.c_void_p), ("colsum", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("Cin", C.c_int32), ("ldx", C.c_int32), ("x_mode", C.c_int32),
        ("c_split", C.c_int32), ("ldx0", C.c_int32),
        ("ksize", C.c_int32), ("Kpad", C.c_int32),
        ("nt", C.c_int32), ("n_slices", C.c_int32),
        ("w_bstride", C.c_int64),
        ("n_store", C.c_int32),
        ("ldo", C.c_int32), ("out_mode", C.c_int32), ("act", C.c_int32),
        ("ldr1", C.c_int32), ("ldr2", C.c_int32), ("r2scale_bstride", C.c_int32),
        ("ps_r", C.c_int32),
        ("in_scale", C.c_float), ("out_scale", C.c_float),
        ("mean", C.c_float * 4),
        ("dtype", C.c_int32),
        ("ld_ln", C.c_int32), ("ln_ones", C.c_int32),
        ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("ln_out", C.c_void_p),
        ("gap_out", C.c_void_p), ("n16_out", C.c_void_p), ("gap_c", C.c_int32), ("reserved0", C.c_int32),
    ]


class HatMlpDesc(C.Structure):
    """Mirror of `struct HatMlpDesc` (include/hat_mi355x.h)."""
    _fields_ = [
        ("x", C.c_void_p), ("w1f", C.c_void_p), ("b1", C.c_void_p), ("w2f", C.c_void_p), ("b2", C.c_void_p),
        ("r1", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("hidden", C.c_int32),
        ("ldx", C.c_int32), ("ldr1", C.c_int32), ("ldo", C.c_int32),
        ("out_f32", C.c_int32), ("dtype", C.c_int32),
    ]


class HatFfnDesc(C.Structure):
    """Mirror of `struct HatFfnDesc` (include/hat_mi355x.h)."""
    _fields_ = [
        ("t_in", C.c_void_p), ("t_out", C.c_void_p), ("ln_g", C.c_void_p), ("ln_b", C.c_void_p),
        ("w1f", C.c_void_p), ("b1", C.c_void_p), ("dww", C.c_void_p), ("dwb", C.c_void_p),
        ("w2f", C.c_void_p), ("b2", C.c_void_p), ("ln1_g", C.c_void_p), ("ln1_b", C.c_void_p),
        ("n_out", C.c_void_p), ("gap_out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("chunks", C.c_int32), ("ldn", C.c_int32), ("gap_c", C.c_int32), ("dtype", C.c_int32),
        ("ldm_in", C.c_int32), ("m_in", C.c_void_p), ("n16_out", C.c_void_p),
    ]


class HatHabTailDesc(C.Structure):
    """Mirror of `struct HatHabTailDesc` (include/hat_mi355x.h)."""
    _fields_ = [("ffn", HatFfnDesc), ("n", C.c_void_p), ("y16", C.c_void_p), ("c1", C.c_void_p), ("w_aggr", C.c_void_p),
                ("wf", C.c_void_p), ("bias_b", C.c_void_p), ("ldn_in", C.c_int32), ("ldr2", C.c_int32), ("r2", C.c_void_p),
                ("r2scale", C.c_void_p), ("r2scale_bstride", C.c_int32), ("reserved1", C.c_int32)]


class HatCabFoldDesc(C.Structure):
    """Mirror of `struct HatCabFoldDesc` (include/hat_mi355x.h)."""
    _fields_ = [
        ("c1", C.c_void_p), ("c1_colsum", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("wk", C.c_void_p),
        ("bias_in", C.c_void_p), ("scale", C.c_void_p), ("wf", C.c_void_p), ("bias_out", C.c_void_p), ("tmp", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("mid", C.c_int32), ("ld1", C.c_int32),
        ("tiles", C.c_int32), ("ldcs", C.c_int32), ("k", C.c_int32), ("ld_scale", C.c_int32), ("dtype", C.c_int32),
        ("conv_scale", C.c_float), ("stats", C.c_void_p), ("w2f", C.c_void_p),
    ]


class HatAggrCabDesc(C.Structure):
    """Mirror of `struct HatAggrCabDesc` (include/hat_mi355x.h)."""
    _fields_ = [("lin", HatConvDesc), ("c1", C.c_void_p), ("wf", C.c_void_p), ("bias_b", C.c_void_p)]


class HatYuvSurface(C.Structure):
    """Mirror of `HatYuvSurface` (include/hat_mi355x.h): one frame surface of any subsampling; bytes everywhere, cb = cr = None: grey."""
    _fields_ = [("y", C.c_void_p), ("y_pitch", C.c_int64), ("y_bstride", C.c_int64), ("cb", C.c_void_p), ("cr", C.c_void_p),
                ("c_pitch", C.c_int64), ("c_step", C.c_int32), ("c_bstride", C.c_int64),
                ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("depth", C.c_int32), ("msb", C.c_int32)]


class HatPackedSurface(C.Structure):
    """Mirror of `HatPackedSurface` (include/hat_mi355x.h): one packed 4:2:2 surface; bytes everywhere, layout: the index in yuv.PACKED_FORMATS."""
    _fields_ = [("base", C.c_void_p), ("pitch", C.c_int64), ("bstride", C.c_int64), ("layout", C.c_int32), ("depth", C.c_int32),
                ("msb", C.c_int32), ("reserved", C.c_int32)]


class HatNafHalfDesc(C.Structure):
    """Mirror of `struct HatNafHalfDesc` (include/hat_mi355x.h)."""
    _fields_ = [("r_in", C.c_void_p), ("gprev", C.c_void_p), ("wf", C.c_void_p), ("bf", C.c_void_p), ("r_out", C.c_void_p),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("dww", C.c_void_p), ("dwb", C.c_void_p), ("g_out", C.c_void_p),
                ("partials", C.c_void_p), ("wf_bstride", C.c_int64), ("bf_bstride", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("ldr", C.c_int32), ("ldg", C.c_int32),
                ("ldo", C.c_int32), ("dtype", C.c_int32), ("reserved0", C.c_int32)]


class HatNafFoldDesc(C.Structure):
    """Mirror of `struct HatNafFoldDesc` (include/hat_mi355x.h)."""
    _fields_ = [("partials", C.c_void_p), ("wsca", C.c_void_p), ("bsca", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("beta", C.c_void_p), ("wf", C.c_void_p), ("bf", C.c_void_p), ("npix", C.c_int64),
                ("B", C.c_int32), ("tiles", C.c_int32), ("C", C.c_int32), ("dtype", C.c_int32)]


class HatEscConvFfnDesc(C.Structure):
    """Mirror of `struct HatEscConvFfnDesc` (include/hat_mi355x.h)."""
    _fields_ = [("x", C.c_void_p), ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("dww", C.c_void_p), ("dwb", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("r", C.c_void_p),
                ("out", C.c_void_p), ("partials", C.c_void_p), ("ln_eps", C.c_float),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("hid_p", C.c_int32), ("ldx", C.c_int32), ("ldr", C.c_int32),
                ("ldo", C.c_int32), ("out_f32", C.c_int32), ("dtype", C.c_int32), ("reserved0", C.c_int32)]


class HatVggConvDesc(C.Structure):
    """Mirror of `struct HatVggConvDesc` (include/hat_mi355x.h)."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("slope", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ldx", C.c_int32), ("ldo", C.c_int32), ("frame", C.c_int32),
                ("dtype", C.c_int32), ("reserved0", C.c_int32)]


class HatRdbConvDesc(C.Structure):
    """Mirror of `struct HatRdbConvDesc` (include/hat_mi355x.h)."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("r1", C.c_void_p), ("r2", C.c_void_p),
                ("s_out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("ldx", C.c_int32), ("ldo", C.c_int32), ("out_off", C.c_int32), ("slope", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("dtype", C.c_int32)]


class HatHeadDesc(C.Structure):
    """Mirror of `struct HatHeadDesc` (include/hat_mi355x.h)."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("ln0_g", C.c_void_p), ("ln0_b", C.c_void_p),
                ("ln1_g", C.c_void_p), ("ln1_b", C.c_void_p), ("f0", C.c_void_p), ("t", C.c_void_p), ("n", C.c_void_p),
                ("n16", C.c_void_p), ("gap_partial", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("Kpad", C.c_int32), ("ldn", C.c_int32), ("gap_c", C.c_int32), ("dtype", C.c_int32), ("in_scale", C.c_float),
                ("mean", C.c_float * 4), ("reserved0", C.c_int32)]


_YUV_BLOCK = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64]   # a 4:2:0 frame block

# name -> (restype, argtypes); every symbol declared in include/hat_mi355x.h
SIGNATURES = {
    "hat_abi_version": (C.c_int, []),
    "hat_target_arch": (C.c_char_p, []),
    "hat_conv_tiles": (C.c_int, [C.POINTER(HatConvDesc), C.POINTER(C.c_int32)]),
    "hat_ocab_mlp": (C.c_int, [C.POINTER(HatMlpDesc), C.c_void_p]),
    "hat_ocab_qkv": (C.c_int, [C.POINTER(HatMlpDesc), C.c_void_p]),
    "hat_conv_occupancy": (C.c_int, [C.POINTER(HatConvDesc), C.POINTER(C.c_int32)]),
    "hat_conv_plan": (C.c_int, [C.POINTER(HatConvDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64)]),
    "hat_conv": (C.c_int, [C.POINTER(HatConvDesc), C.c_void_p]),
    "hat_linear": (C.c_int, [C.POINTER(HatConvDesc), C.c_void_p]),
    # the FP16-range guard: the launch, then the uint32 device slot, then the stream
    "hat_conv_guarded": (C.c_int, [C.POINTER(HatConvDesc), C.c_void_p, C.c_void_p]),
    "hat_linear_guarded": (C.c_int, [C.POINTER(HatConvDesc), C.c_void_p, C.c_void_p]),
    "hat_hab_tail3_guarded": (C.c_int, [C.POINTER(HatHabTailDesc), C.c_void_p, C.c_void_p]),
    "hat_conv3x3_small_groups": (C.c_int, [C.POINTER(HatConvDesc), C.POINTER(C.c_int32)]),
    "hat_conv3x3_small": (C.c_int, [C.POINTER(HatConvDesc), C.c_void_p]),
    "hat_cab_fold": (C.c_int, [C.POINTER(HatCabFoldDesc), C.c_void_p]),
    "hat_aggr_cab": (C.c_int, [C.POINTER(HatAggrCabDesc), C.c_void_p]),
    "hat_ffn_tiles": (C.c_int, [C.POINTER(HatFfnDesc), C.POINTER(C.c_int32)]),
    "hat_ffn": (C.c_int, [C.POINTER(HatFfnDesc), C.c_void_p]),
    "hat_ffn2": (C.c_int, [C.POINTER(HatFfnDesc), C.c_void_p]),
    "hat_hab_tail": (C.c_int, [C.POINTER(HatHabTailDesc), C.c_void_p]),
    "hat_hab_tail3": (C.c_int, [C.POINTER(HatHabTailDesc), C.c_void_p]),
    "hat_plan_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "hat_plan_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "hat_plan_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hat_plan_free": (None, [C.c_void_p]),
    "hat_layernorm_blocks": (C.c_int, []),
    "hat_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_rect_sum": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hat_add_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "hat_esc_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_esc_conv13": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_eca_scale": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_dwconv_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_ocab_keybias": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 9 + [C.c_void_p]),
    "hat_ocab_attention_kb": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 12 + [C.c_void_p]),
    "hat_sgfn_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_ocab_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p]),
    "hat_ocab_attention_log2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p]),
    "hat_cab_squeeze_units": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "hat_cab_squeeze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_conv3x3_to_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]),
    "hat_u8_to_planes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_void_p]),
    "hat_planes_to_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_void_p]),
    "hat_conv3x3_to_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_plan_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                      C.c_void_p]),
    # frame block: y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride
    "hat_yuv420_to_planes": (C.c_int, _YUV_BLOCK + [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "hat_planes_to_yuv420": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + _YUV_BLOCK + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "hat_conv3x3_to_yuv420": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _YUV_BLOCK + [C.c_int32] * 7 + [C.c_float, C.c_void_p, C.c_void_p,
                                                                                                      C.c_int32, C.c_void_p]),
    "hat_plan_forward_yuv420": (C.c_int, [C.c_void_p] + _YUV_BLOCK + [C.c_int32, C.c_int32] + _YUV_BLOCK + [C.c_void_p, C.c_void_p, C.c_void_p]),
    # the deep forms: the same lists with 16-bit blocks, then depth, msb
    "hat_yuv420p16_to_planes": (C.c_int, _YUV_BLOCK + [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                       C.c_int32, C.c_void_p]),
    "hat_planes_to_yuv420p16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + _YUV_BLOCK + [C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                                                                     C.c_int32, C.c_void_p]),
    "hat_conv3x3_to_yuv420p16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _YUV_BLOCK + [C.c_int32] * 7 + [C.c_float, C.c_void_p, C.c_void_p,
                                                                                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_plan_forward_yuv420_deep": (C.c_int, [C.c_void_p] + _YUV_BLOCK + [C.c_int32] * 4 + _YUV_BLOCK + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                                                                     C.c_void_p]),
    # any subsampling: one HatYuvSurface per side
    "hat_yuv_to_planes": (C.c_int, [C.POINTER(HatYuvSurface), C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "hat_planes_to_yuv": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HatYuvSurface), C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p]),
    "hat_conv3x3_to_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HatYuvSurface)] + [C.c_int32] * 7 + [C.c_float, C.c_void_p,
                                                                                                        C.c_void_p, C.c_int32, C.c_void_p]),
    # the folded network ending (hat_upfold.hip): x, wpk, bias, destination, B, H, W, ldx, ..., out_scale, the RGB mean as three floats
    "hat_upfold_to_planes": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_float] * 4 + [C.c_int32, C.c_void_p]),
    "hat_upfold_to_u8": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_int32] * 6 + [C.c_float] * 4 + [C.c_int32, C.c_int32, C.c_void_p]),
    "hat_upfold_to_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HatYuvSurface)] + [C.c_int32] * 6 + [C.c_float] * 4
                          + [C.c_void_p, C.c_int32, C.c_void_p]),
    "hat_plan_forward_yuv": (C.c_int, [C.c_void_p, C.POINTER(HatYuvSurface), C.POINTER(HatYuvSurface), C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    # chroma siting: the surface entries with a siting code (0 centre, 1 left, 2 top-left) beside each surface
    "hat_yuv_to_planes_sited": (C.c_int, [C.POINTER(HatYuvSurface), C.c_int32, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "hat_planes_to_yuv_sited": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HatYuvSurface), C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    "hat_plan_forward_yuv_sited": (C.c_int, [C.c_void_p, C.POINTER(HatYuvSurface), C.c_int32, C.POINTER(HatYuvSurface), C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # packed 4:2:2: one HatPackedSurface per side, the siting beside it; the plan entry takes a packed and a planar pointer a side
    "hat_packed422_to_planes": (C.c_int, [C.POINTER(HatPackedSurface), C.c_int32, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "hat_planes_to_packed422": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HatPackedSurface), C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    "hat_plan_forward_packed422": (C.c_int, [C.c_void_p, C.POINTER(HatPackedSurface), C.POINTER(HatYuvSurface), C.c_int32, C.POINTER(HatPackedSurface),
                                             C.POINTER(HatYuvSurface), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hat_imresize_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "hat_imresize_cols_to_planes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_imresize_cols_to_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "hat_u8_metrics_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "hat_u8_metrics": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hat_pil_resize_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "hat_arb_psnr_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "hat_arb_psnr": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "hat_dihedral_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                   C.c_void_p]),
    "hat_window_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p]),
    "hat_niqe_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int64)]),
    "hat_niqe_y_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "hat_imresize_plane_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_int64, C.c_void_p]),
    "hat_imresize_plane_cols": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "hat_niqe_block_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p,
                                       C.c_void_p]),
    "hat_naf_half_tiles": (C.c_int, [C.c_int32, C.c_int32]),
    "hat_naf_half": (C.c_int, [C.POINTER(HatNafHalfDesc), C.c_void_p]),
    "hat_naf_fold": (C.c_int, [C.POINTER(HatNafFoldDesc), C.c_void_p]),
    "hat_esc_convffn_tiles": (C.c_int, [C.c_int32, C.c_int32]),
    "hat_esc_convffn": (C.c_int, [C.POINTER(HatEscConvFfnDesc), C.c_void_p]),
    "hat_window_attention_r": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 10 + [C.c_void_p]),
    "hat_esc_layernorm": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_esc_shuffle_add": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p]),
    "hat_escreal_skip": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 6 + [C.c_void_p]),
    "hat_dysample": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    "hat_unshuffle_pad": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "hat_escrealm_skip": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] * 8 + [C.c_void_p]),
    "hat_shuffle_planes": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "hat_escfp_convffn": (C.c_int, [C.POINTER(HatEscConvFfnDesc), C.c_void_p]),
    "hat_escfp_layernorm": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_escfp_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32] * 3 + [C.c_void_p]),
    "hat_escfp_shuffle_bicubic": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    "hat_lte_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 11
                      + [C.c_int64, C.c_int32, C.c_int32] + [C.c_float] * 4 + [C.c_void_p, C.c_int32, C.c_void_p]),
    # grid mode into bytes / a YCbCr surface: hat_lte_query's arguments up to b4, then the grid, the cell, the affine and the sink
    "hat_lte_query_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9
                         + [C.c_int32, C.c_int32] + [C.c_float] * 4 + [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "hat_lte_query_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9
                          + [C.c_int32, C.c_int32] + [C.c_float] * 4 + [C.POINTER(HatYuvSurface), C.c_void_p, C.c_int32, C.c_void_p]),
    # the shuffle heads into a frame: rows, ld, base, B, H, W, s, then the sink, the crop and the stream
    "hat_shuffle_to_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 3
                          + [C.c_void_p]),
    "hat_shuffle_to_yuv": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(HatYuvSurface), C.c_int32, C.c_int32,
                                                                                              C.c_void_p, C.c_void_p]),
    "hat_vgg_conv": (C.c_int, [C.POINTER(HatVggConvDesc), C.c_void_p]),
    "hat_vgg_conv_tiles": (C.c_int, [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 3),
    "hat_rdb_conv": (C.c_int, [C.POINTER(HatRdbConvDesc), C.c_void_p]),
    "hat_rdb_conv_tiles": (C.c_int, [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 3),
    "hat_head_fused": (C.c_int, [C.POINTER(HatHeadDesc), C.c_void_p]),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load the library (once) and bind every entry point; raise if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP kernels are not built. Run `python -m super_resolution_amd.build` "
                "(needs hipcc). There is no CPU fallback for the HAT forward pass.")
        # Load PyTorch's HIP runtime FIRST.  torch links "libamdhip64.so" (its bundled copy, found through
        # its own RPATH) while this library links "libamdhip64.so.7": if ours were loaded first the process
        # would end up with two HIP runtimes and our launches would target the one torch never initialised
        # (hipErrorNoDevice).  With torch's copy resident, our NEEDED entry resolves to it by SONAME.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise RuntimeError(f"{LIB_PATH} does not export `{name}` (stale build?)")
            fn.restype = res
            fn.argtypes = args
        if lib.hat_abi_version() != ABI_VERSION:
            raise RuntimeError(f"ABI version mismatch: library {lib.hat_abi_version()}, binding {ABI_VERSION} (stale or overridden "
                               f"{LIB_PATH}? rebuild with `python -m super_resolution_amd.build`)")
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = _ERRORS.get(rc, f"hipError_t {rc}")
        raise RuntimeError(f"{what} failed: {msg}")
