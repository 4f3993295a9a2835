// hat_esc_sink.hip — where the shuffle heads of the ESC family end in a frame instead of in fp32 planes: PixelShuffle(s) of the
// fp32 rows `to_img` left (plus ESC's base image) stored as interleaved bytes or as a YCbCr surface; no fp32 image is written.
// Contract: include/hat_mi355x.h (hat_shuffle_to_u8, hat_shuffle_to_yuv); DESIGN.md 4.21.
// The value of output pixel (b, c, Y, X) is rows[b][Y / s][X / s][c s^2 + (Y % s) s + X % s] (+ base[b][c][Y / s][X / s], one
// rounded fp32 add: what esc_shuffle_add_kernel stores).  It is converted and stored by rgb4_store_u8 and yuv_store_tile
// (hat_frame_sink.h), the functions planes_to_u8_kernel (hat_u8.hip) and planes_to_yuv420_kernel (hat_yuv.hip) end in, with their
// thread shapes: the bytes are those of hat_esc_shuffle_add / hat_shuffle_planes followed by hat_planes_to_u8 / hat_planes_to_yuv.
// Bound: the rows read (4 r4(3 s^2) bytes per LR pixel; every 64-byte line of it is fetched from HBM once and again from L2 by
// the s output rows that share it) and the byte store.  No LDS, no MFMA.
#include "hat_frame_sink.h"

namespace {

struct ShuffleSrc {
    const float* rows;
    const float* base;   // null: no base image
    int H, W, s, ld;
};

// the R x 4 tile of output pixels at (y, x) of sample b: v[j][i][c], zero for the columns i >= n.  With s = 3 the four columns
// straddle LR pixels, so every column has its own (X / s, X % s): one division for the first, steps for the rest.  All loads of
// the tile are issued before the first add (the base image's too), so the thread waits for memory once, not once per value.
template <int R> __device__ __forceinline__ void shuffle_tile(const ShuffleSrc& a, int b, int y, int x, int n, float (&v)[R][4][3]) {
    const float* __restrict__ rows = a.rows;
    const float* __restrict__ base = a.base;
    const bool with_base = base != nullptr;
    const int ss = a.s * a.s, xx0 = x / a.s, ix0 = x - xx0 * a.s;
    const int plane = a.H * a.W;   // (the host checks that it fits; the row index below is 64-bit)
    float bs[R][4][3];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int Y = y + j, yy = Y / a.s, iy = Y - yy * a.s;
        const int64_t prow = ((int64_t)b * a.H + yy) * a.W;
        const float* brow = with_base ? base + (int64_t)b * 3 * plane + (int64_t)yy * a.W : nullptr;
        int xx = xx0, ix = ix0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = i < n;
            const float* r = rows + (prow + xx) * a.ld + iy * a.s + ix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[j][i][c] = in ? r[c * ss] : 0.f;
                bs[j][i][c] = in && with_base ? brow[(int64_t)c * plane + xx] : 0.f;
            }
            if (++ix == a.s) ix = 0, ++xx;
        }
    }
    if (with_base) {
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i < n) v[j][i][c] = hat_add_rn(v[j][i][c], bs[j][i][c]);
    }
}

// one thread = four consecutive pixels of an output row, stored by rgb4_store_u8
__global__ __launch_bounds__(256) void shuffle_to_u8_kernel(const ShuffleSrc a, uint8_t* __restrict__ dst, long long pitch, long long dbstride,
                                                            int w_out, int bgr) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
    if (x >= w_out) return;
    const int n = min(4, w_out - x);
    float v[1][4][3];
    shuffle_tile<1>(a, b, y, x, n, v);
    rgb4_store_u8(dst + (size_t)b * dbstride + (size_t)y * pitch + (size_t)x * 3, v[0], n, bgr);
}

// one thread = (1 + SUB_Y) rows x four columns, converted and stored by yuv_store_tile
template <typename T, int SUB_X, int SUB_Y, bool GREY>
__global__ __launch_bounds__(256) void shuffle_to_yuv_kernel(const ShuffleSrc a, const HatYuvDst<T> d, int w_out, HatCsc k, HatSample<T> q) {
    constexpr int R = 1 + SUB_Y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y * R, b = blockIdx.z;
    if (x >= w_out) return;
    const int n = min(4, w_out - x);
    yuv_store_tile<T, SUB_X, SUB_Y, GREY>(d, k, q, b, y, x, n, [&](float (&rgb)[R][4][3]) { shuffle_tile<R>(a, b, y, x, n, rgb); });
}

// what both entries ask of the source and the crop; 0 when they hold
int shuffle_check(const float* rows, int32_t ld, int32_t B, int32_t H, int32_t W, int32_t s, int32_t h_out, int32_t w_out) {
    if (!rows || (reinterpret_cast<uintptr_t>(rows) & 3) || B < 1 || B > 65535 || H < 1 || W < 1 || s < 1) return HAT_EINVAL;
    if ((int64_t)H * W > INT32_MAX) return HAT_EINVAL;   // (a plane's pixel count is an int in the kernel)
    if (s > 8) return HAT_EUNSUPPORTED;   // hat_esc_shuffle_add's and hat_shuffle_planes' range
    if (ld < 3 * s * s || h_out < 1 || w_out < 1 || h_out > (int64_t)s * H || w_out > (int64_t)s * W || h_out > 65535) return HAT_EINVAL;
    return 0;
}

}  // namespace

extern "C" int hat_shuffle_to_u8(const float* rows, int32_t ld, const float* base, int32_t B, int32_t H, int32_t W, int32_t s, uint8_t* dst,
                                 int64_t dst_pitch, int64_t dst_bstride, int32_t h_out, int32_t w_out, int32_t bgr, void* stream) {
    if (!dst || (reinterpret_cast<uintptr_t>(base) & 3)) return HAT_EINVAL;
    if (const int rc = shuffle_check(rows, ld, B, H, W, s, h_out, w_out)) return rc;
    if (dst_pitch < 3 * (int64_t)w_out || (B > 1 && dst_bstride < dst_pitch * (int64_t)(h_out - 1) + 3 * (int64_t)w_out)) return HAT_EINVAL;
    HAT_LAUNCH(shuffle_to_u8_kernel, dim3((w_out + 1023) / 1024, h_out, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
               ShuffleSrc{rows, base, H, W, s, ld}, dst, (long long)dst_pitch, (long long)dst_bstride, w_out, bgr ? 1 : 0);
    return hat_check_launch();
}

extern "C" int hat_shuffle_to_yuv(const float* rows, int32_t ld, const float* base, int32_t B, int32_t H, int32_t W, int32_t s,
                                  const HatYuvSurface* dst, int32_t h_out, int32_t w_out, const float* from_rgb12, void* stream) {
    if (!dst || !from_rgb12 || (reinterpret_cast<uintptr_t>(base) & 3)) return HAT_EINVAL;
    if (const int rc = shuffle_check(rows, ld, B, H, W, s, h_out, w_out)) return rc;
    if (!hat_yuv_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;   // (odd crops on subsampled axes, short or odd pitches)
    yuv_dispatch(*dst, [&](auto L, auto q) {
        using T = typename decltype(L)::sample_t;
        HAT_LAUNCH((shuffle_to_yuv_kernel<T, L.sx, L.sy, L.grey>), dim3((w_out + 1023) / 1024, h_out >> L.sy, B), dim3(256), 0,
                   reinterpret_cast<hipStream_t>(stream), ShuffleSrc{rows, base, H, W, s, ld}, yuv_dst<T>(*dst), w_out, load_csc(from_rgb12), q);
    });
    return hat_check_launch();
}
