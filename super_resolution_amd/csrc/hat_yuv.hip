// hat_yuv.hip — the 4:2:0 frame boundary: 8-bit YCbCr frames (NV12 / NV21 / I420) <-> the network's fp32 RGB planes.
// Contract: include/hat_mi355x.h (hat_yuv420_to_planes, hat_planes_to_yuv420); definition: super_resolution_amd/yuv.py;
// colour conversion: basicsr utils/color_util.py (rgb2ycbcr, ycbcr2rgb: BT.601, 16-235), shared with conv_last's yuv epilogue
// through hat_common.h (hat_ycc_to_rgb, hat_rgb_to_ycc).  cb and cr are separate pointers with a byte step between the
// samples of a row (1: planar, 2: interleaved), so one kernel serves all three layouts.
#include "hat_common.h"
#include "hat_yuv_check.h"

namespace {

// one thread = one pixel of the padded plane row (hat_u8_to_planes' shape): a Y byte, the Cb and Cr bytes of its 2 x 2 block
// (the four pixels of a block read the same two bytes: L1), three plane stores coalesced over the lanes.  Reflection as in
// u8_to_planes_kernel; the chroma sample of source pixel (sy, sx) is (sy >> 1, sx >> 1).
__global__ __launch_bounds__(256) void yuv420_to_planes_kernel(const uint8_t* __restrict__ yp, long long y_pitch, long long y_bstride,
                                                               const uint8_t* __restrict__ cbp, const uint8_t* __restrict__ crp,
                                                               long long c_pitch, int c_step, long long c_bstride, float* __restrict__ dst,
                                                               int h, int w, int Hp, int Wp, HatCsc k) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    const size_t co = (size_t)b * c_bstride + (size_t)(sy >> 1) * c_pitch + (size_t)(sx >> 1) * c_step;
    float rgb[3];
    hat_ycc_to_rgb(k, yp[(size_t)b * y_bstride + (size_t)sy * y_pitch + sx], cbp[co], crp[co], rgb);
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = rgb[c];
}

// one thread = two rows x four columns = two 2 x 2 blocks: rows are not independent here.  Per row and plane 16 contiguous
// bytes are loaded; the Y bytes of a row go out as one dword where the segment is whole and 4-byte aligned, as single bytes
// otherwise; the two Cb and two Cr bytes are single byte stores (planar or interleaved: the step decides).
__global__ __launch_bounds__(256) void planes_to_yuv420_kernel(const float* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ yp,
                                                               long long y_pitch, long long y_bstride, uint8_t* __restrict__ cbp,
                                                               uint8_t* __restrict__ crp, long long c_pitch, int c_step, long long c_bstride,
                                                               int w_out, HatCsc k) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y * 2, b = blockIdx.z;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* s = src + (size_t)b * 3 * plane + (size_t)y * Ws + x;
    const int n = min(4, w_out - x);          // 2 or 4: w_out is even
    float cb[2][4], cr[2][4];
    unsigned q[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float Y = 0.f;
            cb[j][i] = cr[j][i] = 0.f;
            if (i < n) hat_rgb_to_ycc(k, s[(size_t)j * Ws + i], s[plane + (size_t)j * Ws + i], s[2 * plane + (size_t)j * Ws + i], Y, cb[j][i], cr[j][i]);
            q[j][i] = hat_ycc_byte(Y);
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint8_t* o = yp + (size_t)b * y_bstride + (size_t)(y + j) * y_pitch + x;
        if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<unsigned*>(o) = q[j][0] | (q[j][1] << 8) | (q[j][2] << 16) | (q[j][3] << 24);
        } else {
            for (int i = 0; i < n; ++i) o[i] = (uint8_t)q[j][i];
        }
    }
    const size_t co = (size_t)b * c_bstride + (size_t)(y >> 1) * c_pitch + (size_t)(x >> 1) * c_step;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (2 * i < n) {
            cbp[co + (size_t)i * c_step] = (uint8_t)hat_chroma_byte(hat_add_rn(cb[0][2 * i], cb[0][2 * i + 1]), hat_add_rn(cb[1][2 * i], cb[1][2 * i + 1]), k.m[7]);
            crp[co + (size_t)i * c_step] = (uint8_t)hat_chroma_byte(hat_add_rn(cr[0][2 * i], cr[0][2 * i + 1]), hat_add_rn(cr[1][2 * i], cr[1][2 * i + 1]), k.m[11]);
        }
    }
}

HatCsc load_csc(const float* m12) {
    HatCsc k;
    for (int i = 0; i < 12; ++i) k.m[i] = m12[i];
    return k;
}

}  // namespace

extern "C" int hat_yuv420_to_planes(const uint8_t* y, int64_t y_pitch, int64_t y_bstride, const uint8_t* cb, const uint8_t* cr,
                                    int64_t c_pitch, int32_t c_step, int64_t c_bstride, float* dst, int32_t B, int32_t h, int32_t w,
                                    int32_t Hp, int32_t Wp, const float* to_rgb12, void* stream) {
    if (!y || !cb || !cr || !dst || !to_rgb12 || !hat_yuv_block_ok(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h, w)) return HAT_EINVAL;
    if (Hp < h || Wp < w || B > 65535 || Hp > 65535) return HAT_EINVAL;
    if (Hp - h >= h || Wp - w >= w) return HAT_EINVAL;   // the reflection needs a source row / column: pad < size
    HAT_LAUNCH(yuv420_to_planes_kernel, dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y,
               (long long)y_pitch, (long long)y_bstride, cb, cr, (long long)c_pitch, (int)c_step, (long long)c_bstride, dst, h, w, Hp, Wp,
               load_csc(to_rgb12));
    return hat_check_launch();
}

extern "C" int hat_planes_to_yuv420(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint8_t* y, int64_t y_pitch, int64_t y_bstride,
                                    uint8_t* cb, uint8_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t h_out,
                                    int32_t w_out, const float* from_rgb12, void* stream) {
    if (!src || !y || !cb || !cr || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_block_ok(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h_out, w_out))
        return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out / 2 > 65535) return HAT_EINVAL;
    HAT_LAUNCH(planes_to_yuv420_kernel, dim3((w_out + 1023) / 1024, h_out / 2, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
               Hs, Ws, y, (long long)y_pitch, (long long)y_bstride, cb, cr, (long long)c_pitch, (int)c_step, (long long)c_bstride, w_out,
               load_csc(from_rgb12));
    return hat_check_launch();
}
