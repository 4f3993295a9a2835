// hat_yuv_check.h — the host-side checks of a frame block (4:2:0: the first two; any subsampling: hat_yuv_surface_ok) (include/hat_mi355x.h, "The 4:2:0 frame boundary"), shared by
// hat_yuv.hip, hat_cabsq.hip and hat_plan.cpp.  Plain C++ (hat_plan.cpp is not a HIP source and cannot include hat_common.h).
#pragma once
#include <stdint.h>

#include "../../include/hat_mi355x.h"

// sizes, chroma step, pitches and batch strides (bytes) of a (B, h, w) block: even sizes, rows fit their pitch, samples of
// the batch do not overlap (the b-strides are ignored for B == 1); the pointers are the caller's to check
static inline bool hat_yuv_block_ok(int64_t y_pitch, int64_t y_bstride, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t B,
                                    int64_t h, int64_t w) {
    if (B < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || (c_step != 1 && c_step != 2)) return false;
    const int64_t crow = (int64_t)c_step * (w / 2);
    if (y_pitch < w || c_pitch < crow) return false;
    return B == 1 || (y_bstride >= y_pitch * (h - 1) + w && c_bstride >= c_pitch * (h / 2 - 1) + crow);
}

// the same for samples of bps bytes (1: bytes, 2: 16-bit words).  Pitches, strides and c_step stay in BYTES (decoder surfaces
// report bytes): c_step is bps (planar) or 2 bps (interleaved), and with words every pitch and stride that is used is even
static inline bool hat_yuv_block_ok_n(int64_t y_pitch, int64_t y_bstride, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t B,
                                      int64_t h, int64_t w, int32_t bps) {
    if (bps == 1) return hat_yuv_block_ok(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h, w);
    if (bps != 2 || B < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || (c_step != 2 && c_step != 4)) return false;
    const int64_t yrow = 2 * w, crow = (int64_t)c_step * (w / 2);
    if (y_pitch < yrow || c_pitch < crow || (y_pitch & 1) || (c_pitch & 1)) return false;
    return B == 1 || (!(y_bstride & 1) && !(c_bstride & 1) && y_bstride >= y_pitch * (h - 1) + yrow && c_bstride >= c_pitch * (h / 2 - 1) + crow);
}

// sample widths of the deep entries: an n-bit code in a 16-bit little-endian word, MSB-aligned (msb = 1: P010 / P012 / P016) or
// LSB-aligned (msb = 0: yuv420p10le ...); at 16 bits the two are the same
static inline bool hat_yuv_depth_ok(int32_t depth, int32_t msb) { return (depth == 10 || depth == 12 || depth == 16) && (msb == 0 || msb == 1); }

// one HatYuvSurface holding a (B, h, w) block, any subsampling: the sample width, the pointers (cb = cr = NULL: grey, then
// sub_x / sub_y and the chroma fields are not read; one of them NULL is an error; words are 2-byte aligned), the sizes (w even
// where sub_x = 1, h even where sub_y = 1; (sub_x, sub_y) is (1,1), (1,0) or (0,0)), c_step = bps (planar) or 2 bps
// (interleaved), rows that fit their pitch, samples of the batch that do not overlap (the b-strides are ignored for B == 1), and
// with words even pitches and strides
static inline bool hat_yuv_surface_ok(const HatYuvSurface* s, int32_t B, int64_t h, int64_t w) {
    if (!s || !s->y || B < 1 || h < 1 || w < 1 || (s->msb != 0 && s->msb != 1)) return false;
    if (s->depth != 8 && !hat_yuv_depth_ok(s->depth, s->msb)) return false;
    const int64_t bps = s->depth == 8 ? 1 : 2, yrow = bps * w;
    if (!s->cb != !s->cr) return false;
    const bool grey = !s->cb;
    if (bps == 2 && (((uintptr_t)s->y | (uintptr_t)s->cb | (uintptr_t)s->cr) & 1)) return false;
    if (s->y_pitch < yrow || (bps == 2 && (s->y_pitch & 1))) return false;
    if (B > 1 && (s->y_bstride < s->y_pitch * (h - 1) + yrow || (bps == 2 && (s->y_bstride & 1)))) return false;
    if (grey) return true;
    if ((s->sub_x != 0 && s->sub_x != 1) || (s->sub_y != 0 && s->sub_y != 1) || s->sub_y > s->sub_x) return false;   // 4:4:0: out of scope
    if ((s->sub_x && (w & 1)) || (s->sub_y && (h & 1))) return false;
    if (s->c_step != bps && s->c_step != 2 * bps) return false;
    const int64_t crow = (int64_t)s->c_step * (w >> s->sub_x), ch = h >> s->sub_y;
    if (s->c_pitch < crow || (bps == 2 && (s->c_pitch & 1))) return false;
    return B == 1 || (s->c_bstride >= s->c_pitch * (ch - 1) + crow && !(bps == 2 && (s->c_bstride & 1)));
}

// the frame block of a 4:2:0 entry as the surface it is: sub_x = sub_y = 1 (the 8-bit entries pass depth 8, msb 0)
static inline HatYuvSurface hat_yuv420_surface(const void* y, int64_t y_pitch, int64_t y_bstride, const void* cb, const void* cr, int64_t c_pitch,
                                               int32_t c_step, int64_t c_bstride, int32_t depth, int32_t msb) {
    return HatYuvSurface{const_cast<void*>(y), y_pitch, y_bstride, const_cast<void*>(cb), const_cast<void*>(cr), c_pitch, c_step, c_bstride, 1, 1, depth, msb};
}

// chroma siting (include/hat_mi355x.h, "Chroma siting"): a code of HAT_SITING_*, and what a checked surface makes of it — an axis
// is co-sited only where it is subsampled, so 4:4:4 and grey are centre under every siting and 4:2:2 'topleft' is 'left'
static inline bool hat_siting_ok(int32_t siting) { return siting == HAT_SITING_CENTER || siting == HAT_SITING_LEFT || siting == HAT_SITING_TOPLEFT; }

static inline int32_t hat_siting_of(const HatYuvSurface* s, int32_t siting) {
    if (!s->cb || !s->sub_x || siting == HAT_SITING_CENTER) return HAT_SITING_CENTER;
    return siting == HAT_SITING_TOPLEFT && s->sub_y ? HAT_SITING_TOPLEFT : HAT_SITING_LEFT;
}
