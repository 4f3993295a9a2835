// hat_packed_check.h — the host-side checks of a packed 4:2:2 surface (include/hat_mi355x.h, "Packed 4:2:2"), shared by
// hat_packed422.hip and hat_plan.cpp.  Plain C++, like hat_yuv_check.h.
#pragma once
#include <stdint.h>

#include "../../include/hat_mi355x.h"

// the depth a layout takes: 8 for uyvy / yuy2, 10 / 12 / 16 for y210, 10 for v210
static inline bool hat_packed_depth_ok(int32_t layout, int32_t depth) {
    if (layout == HAT_PACKED_UYVY || layout == HAT_PACKED_YUY2) return depth == 8;
    if (layout == HAT_PACKED_Y210) return depth == 10 || depth == 12 || depth == 16;
    return layout == HAT_PACKED_V210 && depth == 10;
}

// bytes of a row of w pixels: 4 per pair of bytes, 8 per pair of words, 128 per 48 pixels (v210 rows end on that quantum)
static inline int64_t hat_packed_row_bytes(int32_t layout, int64_t w) {
    if (layout == HAT_PACKED_V210) return 128 * ((w + 47) / 48);
    return (layout == HAT_PACKED_Y210 ? 4 : 2) * w;
}

// one HatPackedSurface holding a (B, h, w) block: the layout with its depth and msb, w even and >= 2, h >= 1, base and pitch
// aligned to the unit's word (2 bytes for y210, 4 for the others), rows that fit their pitch, frames of the batch that do not
// overlap (bstride, aligned too, is ignored for B == 1)
static inline bool hat_packed_surface_ok(const HatPackedSurface* s, int32_t B, int64_t h, int64_t w) {
    if (!s || !s->base || B < 1 || h < 1 || w < 2 || (w & 1)) return false;
    if (s->layout < HAT_PACKED_UYVY || s->layout > HAT_PACKED_V210 || !hat_packed_depth_ok(s->layout, s->depth)) return false;
    if (s->msb != 0 && s->msb != 1) return false;
    const int64_t row = hat_packed_row_bytes(s->layout, w), align = s->layout == HAT_PACKED_Y210 ? 2 : 4;
    if (((uintptr_t)s->base & (uintptr_t)(align - 1)) || (s->pitch & (align - 1)) || s->pitch < row) return false;
    return B == 1 || (!(s->bstride & (align - 1)) && s->bstride >= s->pitch * (h - 1) + row);
}

// the padded planes hold the frame, fit the grid, and the reflection has a source row / column: pad < size (the planar entries' rule)
static inline bool hat_packed_padded_ok(int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp) {
    return Hp >= h && Wp >= w && B <= 65535 && Hp <= 65535 && Hp - h < h && Wp - w < w;
}
