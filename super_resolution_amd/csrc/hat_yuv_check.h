// hat_yuv_check.h — the one host-side check of a 4:2:0 frame block (include/hat_mi355x.h, "The 4:2:0 frame boundary"), shared by
// hat_yuv.hip, hat_cabsq.hip and hat_plan.cpp.  Plain C++ (hat_plan.cpp is not a HIP source and cannot include hat_common.h).
#pragma once
#include <stdint.h>

// sizes, chroma step, pitches and batch strides (bytes) of a (B, h, w) block: even sizes, rows fit their pitch, samples of
// the batch do not overlap (the b-strides are ignored for B == 1); the pointers are the caller's to check
static inline bool hat_yuv_block_ok(int64_t y_pitch, int64_t y_bstride, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t B,
                                    int64_t h, int64_t w) {
    if (B < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || (c_step != 1 && c_step != 2)) return false;
    const int64_t crow = (int64_t)c_step * (w / 2);
    if (y_pitch < w || c_pitch < crow) return false;
    return B == 1 || (y_bstride >= y_pitch * (h - 1) + w && c_bstride >= c_pitch * (h / 2 - 1) + crow);
}
