// hat_pil_resize.hip — the two device pieces of the ESC-LTE benchmark loop (esc_arb/test.py eval_psnr).
// Contract: include/hat_mi355x.h (hat_pil_resize_u8, hat_arb_psnr, hat_arb_psnr_workspace_bytes); host definitions:
// super_resolution_amd/resize.py (pil_tables, pil_bicubic_u8) and super_resolution_amd/metrics.py (arb_psnr).
//
// hat_pil_resize_u8: Pillow's 8-bit bicubic Image.resize (libImaging/Resample.c), the resize the reference's wrappers make
// their LR images with (esc_arb/datasets/wrappers.py:149-152).  Integer arithmetic only: the host builds 22-bit fixed-point
// coefficients and (first tap, tap count) per output position; a pass is out = clip8((2^21 + sum_k coef[k] * pixel[first + k])
// >> 22) in int32, the horizontal pass into a uint8 intermediate, then the vertical pass.  One thread per output BYTE in both
// passes: adjacent lanes walk adjacent bytes of a row (a lane's taps are 3 bytes apart in the horizontal pass, a row apart in
// the vertical pass, where the 64 lanes of a wave then read 64 consecutive bytes of each tap row).  The grid is capped at
// PR_MAX_BLOCKS workgroups of PR_THREADS threads and loops: a pass takes a second trip above PR_MAX_BLOCKS * PR_THREADS
// output bytes (524288 bytes = 174762 pixels and two thirds).
//
// hat_arb_psnr: utils.py:132-149 (calc_psnr) on the clamped fp32 output against byte / 255, squares accumulated in fp64, one
// partial per workgroup, then a fixed-order finish (hat_u8_metrics' scheme): reproducible bit for bit.
#include <algorithm>

#include "hat_common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_BLOCKS = 2048;
constexpr int PR_BITS = 22;                 // Resample.c: PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ uint8_t clip8(int v) { return (uint8_t)min(max(v >> PR_BITS, 0), 255); }

// The taps of output position `i`: (first, count) cut to what the tables and the source hold, so that a wrong table reads
// nothing outside the source (the library cannot look into device tables before the launch).
__device__ __forceinline__ int taps_of(const int* __restrict__ bounds, int i, int K, int in_len, int* first) {
    const int f = bounds[2 * i], n = bounds[2 * i + 1];
    *first = f;
    return (f < 0 || n < 0 || n > K || (long long)f + n > in_len) ? 0 : n;
}

// src (h, w, 3) uint8, pitched -> mid (h, ow, 3) uint8, packed.  One thread = one byte (y, 3 x + c) of mid.
__global__ __launch_bounds__(PR_THREADS) void pil_resize_h_kernel(const uint8_t* __restrict__ src, long long pitch, int h, int w, int ow,
                                                                  const int* __restrict__ coef, const int* __restrict__ bounds, int K,
                                                                  uint8_t* __restrict__ mid) {
    const long long row = 3LL * ow, total = row * h;
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PR_THREADS) {
        const int y = (int)(i / row), j = (int)(i - (long long)y * row);
        const int x = j / 3, c = j - 3 * x;
        int first;
        const int n = taps_of(bounds, x, K, w, &first);
        const uint8_t* p = src + (size_t)y * pitch + (size_t)first * 3 + c;
        const int* k = coef + (size_t)x * K;
        int acc = 1 << (PR_BITS - 1);
        for (int t = 0; t < n; ++t) acc += k[t] * (int)p[3 * t];
        mid[i] = clip8(acc);
    }
}

// mid (h, ow, 3) uint8, packed -> dst (oh, ow, 3) uint8, pitched.  One thread = one byte (y, j) of dst; bytes past 3 ow of a
// pitched row are not touched.
__global__ __launch_bounds__(PR_THREADS) void pil_resize_v_kernel(const uint8_t* __restrict__ mid, int h, int ow, int oh,
                                                                  const int* __restrict__ coef, const int* __restrict__ bounds, int K,
                                                                  uint8_t* __restrict__ dst, long long pitch) {
    const long long row = 3LL * ow, total = row * oh;
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PR_THREADS) {
        const int y = (int)(i / row), j = (int)(i - (long long)y * row);
        int first;
        const int n = taps_of(bounds, y, K, h, &first);
        const uint8_t* p = mid + (size_t)first * row + j;
        const int* k = coef + (size_t)y * K;
        int acc = 1 << (PR_BITS - 1);
        for (int t = 0; t < n; ++t) acc += k[t] * (int)p[(size_t)t * row];
        dst[(size_t)y * pitch + j] = clip8(acc);
    }
}

int pass_blocks(long long bytes) { return (int)std::min<long long>((bytes + PR_THREADS - 1) / PR_THREADS, PR_MAX_BLOCKS); }

// ---- hat_arb_psnr ----
constexpr int AP_THREADS = 256;
constexpr int AP_MAX_BLOCKS = 1024;

// One thread = one pixel of the shaved core at a time, row-major.  d_c = clamp(pred_c, 0, 1) - byte_c / 255 in fp32; gray:
// ((d_0 k_0 + d_1 k_1) + d_2 k_2) with k = float32(65.738, 129.057, 25.064) / 256, every product and sum rounded on its own.
__global__ __launch_bounds__(AP_THREADS) void arb_psnr_kernel(const float* __restrict__ pred, int ph, int pw, const uint8_t* __restrict__ gt,
                                                              long long pitch, int hc, int wc, int shave, int gray,
                                                              double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[AP_THREADS / 64];
    const long long total = (long long)hc * wc;
    const size_t plane = (size_t)ph * pw;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * AP_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AP_THREADS) {
        const int y = (int)(i / wc), x = (int)(i - (long long)y * wc);
        const float* p = pred + (size_t)(y + shave) * pw + (x + shave);
        const uint8_t* g = gt + (size_t)(y + shave) * pitch + (size_t)(x + shave) * 3;
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = fminf(fmaxf(p[c * plane], 0.f), 1.f) - hat_u8_unit.v[g[c]];
        if (gray) {
            const float v = (d[0] * (65.738f / 256.0f) + d[1] * (129.057f / 256.0f)) + d[2] * (25.064f / 256.0f);
            acc += (double)v * (double)v;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc += (double)d[c] * (double)d[c];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// sums[0] = the partials added in a fixed order (thread t: t, t + 256, ...; then a tree), sums[1] = the number of terms.
__global__ __launch_bounds__(AP_THREADS) void arb_psnr_finish(const double* __restrict__ part, int nblocks, double count,
                                                              double* __restrict__ sums) {
    __shared__ double rd[AP_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < nblocks; i += AP_THREADS) s += part[i];
    rd[t] = s;
    __syncthreads();
    for (int o = AP_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) rd[t] += rd[t + o];
        __syncthreads();
    }
    if (t == 0) {
        sums[0] = rd[0];
        sums[1] = count;
    }
}

struct PsnrGeom {
    int hc, wc, blocks;
};

int psnr_geometry(int32_t h, int32_t w, int32_t shave, PsnrGeom* g) {
    if (h < 1 || w < 1 || shave < 0) return HAT_EINVAL;
    if (2 * (int64_t)shave >= h || 2 * (int64_t)shave >= w) return HAT_EINVAL;   // no pixel is left (shave 0: h, w >= 1 holds)
    g->hc = h - 2 * shave;
    g->wc = w - 2 * shave;
    g->blocks = (int)std::min<int64_t>(((int64_t)g->hc * g->wc + AP_THREADS - 1) / AP_THREADS, AP_MAX_BLOCKS);
    return 0;
}

}  // namespace

extern "C" int hat_pil_resize_u8(const uint8_t* src, int64_t src_pitch, int32_t h, int32_t w, uint8_t* mid, uint8_t* dst, int64_t dst_pitch,
                                 int32_t oh, int32_t ow, const int32_t* coef_w, const int32_t* bounds_w, int32_t K_w, const int32_t* coef_h,
                                 const int32_t* bounds_h, int32_t K_h, void* stream) {
    if (!src || !mid || !dst || !coef_w || !bounds_w || !coef_h || !bounds_h) return HAT_EINVAL;
    if (h < 1 || w < 1 || oh < 1 || ow < 1 || K_w < 1 || K_h < 1) return HAT_EINVAL;
    if (src_pitch < 3 * (int64_t)w || dst_pitch < 3 * (int64_t)ow) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HAT_LAUNCH(pil_resize_h_kernel, dim3(pass_blocks(3LL * ow * h)), dim3(PR_THREADS), 0, s, src, (long long)src_pitch, h, w, ow, coef_w,
               bounds_w, (int)K_w, mid);
    if (int rc = hat_check_launch()) return rc;
    HAT_LAUNCH(pil_resize_v_kernel, dim3(pass_blocks(3LL * ow * oh)), dim3(PR_THREADS), 0, s, mid, h, ow, oh, coef_h, bounds_h, (int)K_h, dst,
               (long long)dst_pitch);
    return hat_check_launch();
}

extern "C" int hat_arb_psnr_workspace_bytes(int32_t h, int32_t w, int32_t shave, int64_t* bytes) {
    PsnrGeom g;
    if (!bytes) return HAT_EINVAL;
    if (int rc = psnr_geometry(h, w, shave, &g)) return rc;
    *bytes = (int64_t)g.blocks * 8;
    return 0;
}

extern "C" int hat_arb_psnr(const float* pred, int32_t ph, int32_t pw, const uint8_t* gt, int64_t gt_pitch, int32_t h, int32_t w,
                            int32_t gray, int32_t shave, double* sums, void* workspace, void* stream) {
    PsnrGeom g;
    if (int rc = psnr_geometry(h, w, shave, &g)) return rc;
    if (!pred || !gt || !sums || !workspace || ph < h || pw < w || gt_pitch < 3 * (int64_t)w) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    HAT_LAUNCH(arb_psnr_kernel, dim3(g.blocks), dim3(AP_THREADS), 0, s, pred, ph, pw, gt, (long long)gt_pitch, g.hc, g.wc, shave, gray ? 1 : 0,
               part);
    if (int rc = hat_check_launch()) return rc;
    HAT_LAUNCH(arb_psnr_finish, dim3(1), dim3(AP_THREADS), 0, s, part, g.blocks, (double)g.hc * g.wc * (gray ? 1 : 3), sums);
    return hat_check_launch();
}
