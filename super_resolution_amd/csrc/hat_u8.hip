// hat_u8.hip — the 8-bit frame boundary: interleaved uint8 frames <-> the network's fp32 planes.
// Contract: include/hat_mi355x.h (hat_u8_to_planes, hat_planes_to_u8); reference: basicsr utils/img_util.py:9-35, :131
// (float32(u8) / 255, HWC -> CHW, BGR -> RGB), hat/models/hat_model.py:16-26 (reflect-pad bottom / right to a window
// multiple), :110-112 (crop) and img_util.py:66-91 (tensor2img: clamp, x255, round half to even, CHW -> HWC).
#include "hat_frame_sink.h"

namespace {

// one thread = one pixel of the padded plane row: three byte loads (the row's bytes stay in L1 / L2 across the 3 reads of
// a lane and the neighbouring lanes), three plane stores coalesced over the lanes.  Reflection (F.pad 'reflect', no edge
// repeat): padded row y >= h reads row 2 (h - 1) - y, likewise in x.
__global__ __launch_bounds__(256) void u8_to_planes_kernel(const uint8_t* __restrict__ src, long long pitch, long long sbstride,
                                                           float* __restrict__ dst, int h, int w, int Hp, int Wp, int bgr) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    const uint8_t* p = src + (size_t)b * sbstride + (size_t)sy * pitch + (size_t)sx * 3;
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = hat_u8_unit.v[p[bgr ? 2 - c : c]];
}

// one thread = four consecutive pixels of an output row = 12 bytes, stored by rgb4_store_u8 (hat_frame_sink.h).  The plane loads
// of a lane are 16 contiguous bytes per plane; a wave covers 1 KB of each plane row.
__global__ __launch_bounds__(256) void planes_to_u8_kernel(const float* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst,
                                                           long long pitch, long long dbstride, int h_out, int w_out, int bgr) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* s = src + (size_t)b * 3 * plane + (size_t)y * Ws + x;
    const int n = min(4, w_out - x);
    float rgb[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[i][c] = i < n ? s[c * plane + i] : 0.f;
    rgb4_store_u8(dst + (size_t)b * dbstride + (size_t)y * pitch + (size_t)x * 3, rgb, n, bgr);
}

}  // namespace

extern "C" int hat_u8_to_planes(const uint8_t* src, int64_t src_pitch, int64_t src_bstride, float* dst, int32_t B, int32_t h,
                                int32_t w, int32_t Hp, int32_t Wp, int32_t bgr, void* stream) {
    if (!src || !dst || B < 1 || h < 1 || w < 1 || Hp < h || Wp < w || B > 65535 || Hp > 65535) return HAT_EINVAL;
    if (src_pitch < 3 * (int64_t)w || (B > 1 && src_bstride < src_pitch * (int64_t)(h - 1) + 3 * (int64_t)w)) return HAT_EINVAL;
    if (Hp - h >= h || Wp - w >= w) return HAT_EINVAL;   // the reflection needs a source row / column: pad < size
    HAT_LAUNCH(u8_to_planes_kernel, dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
               (long long)src_pitch, (long long)src_bstride, dst, h, w, Hp, Wp, bgr ? 1 : 0);
    return hat_check_launch();
}

extern "C" int hat_planes_to_u8(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint8_t* dst, int64_t dst_pitch,
                                int64_t dst_bstride, int32_t h_out, int32_t w_out, int32_t bgr, void* stream) {
    if (!src || !dst || B < 1 || Hs < 1 || Ws < 1 || h_out < 1 || w_out < 1 || h_out > Hs || w_out > Ws || B > 65535 || h_out > 65535)
        return HAT_EINVAL;
    if (dst_pitch < 3 * (int64_t)w_out || (B > 1 && dst_bstride < dst_pitch * (int64_t)(h_out - 1) + 3 * (int64_t)w_out)) return HAT_EINVAL;
    HAT_LAUNCH(planes_to_u8_kernel, dim3((w_out + 1023) / 1024, h_out, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
               Hs, Ws, dst, (long long)dst_pitch, (long long)dst_bstride, h_out, w_out, bgr ? 1 : 0);
    return hat_check_launch();
}
