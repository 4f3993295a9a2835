// hat_niqe.hip — the device side of NIQE (basicsr metrics/niqe.py): rounded BT.601 Y plane, one-plane bicubic half-size, and
// per block the 25 sums the AGGD fits need.  Contract: include/hat_mi355x.h (hat_niqe_*, hat_imresize_plane_*); definition:
// super_resolution_amd/niqe.py, which restates the reference in its dtypes.  The reference runs in float32: scipy's convolve
// adds the 49 taps in a double in raster order and rounds mu and conv(img^2) to float32, and sigma = sqrt(|conv(img^2) - mu^2|)
// is then a float32 cancellation.  The block kernel does exactly that (contraction off), so its maps equal niqe.py's bit for
// bit; only the order of the final fp64 sums differs.
//
// Layout: one workgroup of 256 threads per block.  The (block + 6)^2 input patch is staged in LDS with
// coordinates clamped to the IMAGE edge (`nearest`), n of the block is written to LDS (36 KB at 96^2), and the five maps'
// sums are taken from there with np.roll's wrap inside the block.  78.5 KB of LDS at 96^2: two workgroups per CU.  Nothing
// but the 25 doubles leaves the workgroup.
#include "hat_common.h"

namespace {

constexpr int NQ_T = 256;
constexpr int NQ_BLOCK = 96;   // the reference's block; the second scale uses NQ_BLOCK / 2

struct NiqeWindow { double w[49]; };

// metrics.to_y_channel of one pixel, as hat_metrics.hip's y_value forms it (fp64 dot product in numpy's order, float32(y / 255)
// * 255 in fp32), then niqe.py's round(): half to even
__device__ __forceinline__ float y_rounded(const uint8_t* p, int bgr) {
#pragma clang fp contract(off)
    const double r = (double)hat_u8_unit.v[p[bgr ? 2 : 0]], g = (double)hat_u8_unit.v[p[1]], b = (double)hat_u8_unit.v[p[bgr ? 0 : 2]];
    const double y = ((r * 65.481 + g * 128.553) + b * 24.966) + 16.0;
    const float f = (float)(y / 255.0);
    return __builtin_rintf(f * 255.0f);
}

__global__ __launch_bounds__(NQ_T) void niqe_y_kernel(const uint8_t* __restrict__ src, long long pitch, long long bstride, int crop,
                                                      int H, int W, int bgr, float* __restrict__ plane, float* __restrict__ unit) {
    const int x = blockIdx.x * NQ_T + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const float v = y_rounded(src + (size_t)b * bstride + (size_t)(crop + y) * pitch + (size_t)(crop + x) * 3, bgr);
    const size_t o = ((size_t)b * H + y) * W + x;
    plane[o] = v;
    if (unit) unit[o] = hat_u8_unit.v[min(max((int)v, 0), 255)];   // float32(v) / 255: v is a level (16..235)
}

__device__ __forceinline__ float mac_rn(float acc, float w, float v) {   // hat_resize.hip's: acc + w * v as two roundings
#pragma clang fp contract(off)
    const float p = w * v;
    return acc + p;
}

// resize.py's H pass of one plane per sample: one thread = one source column of one output row
__global__ __launch_bounds__(NQ_T) void plane_rows_kernel(const float* __restrict__ src, float* __restrict__ mid, const float* __restrict__ wt,
                                                          const int* __restrict__ st, int P, int h, int w, int oh) {
    const int x = blockIdx.x * NQ_T + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (x >= w) return;
    const float* p = src + (size_t)b * h * w + x;
    float acc = 0.f;
    for (int k = 0; k < P; ++k) acc = mac_rn(acc, wt[(size_t)i * P + k], p[(size_t)st[(size_t)i * P + k] * w]);
    mid[((size_t)b * oh + i) * w + x] = acc;
}

// the W pass; the result times out_scale (its own rounding: niqe.py's `* 255.`)
__global__ __launch_bounds__(NQ_T) void plane_cols_kernel(const float* __restrict__ mid, int w, int oh, int ow, const float* __restrict__ wt,
                                                          const int* __restrict__ st, int P, float out_scale, float* __restrict__ dst) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * NQ_T + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= ow) return;
    const float* m = mid + ((size_t)b * oh + y) * w;
    float acc = 0.f;
    for (int k = 0; k < P; ++k) acc = mac_rn(acc, wt[(size_t)x * P + k], m[st[(size_t)x * P + k]]);
    dst[((size_t)b * oh + y) * ow + x] = acc * out_scale;
}

// One workgroup = one block x block tile of one sample.  smem: patch[(BS + 6)^2] then n[BS^2], floats.
template <int BS>
__global__ __launch_bounds__(NQ_T) void niqe_block_kernel(const float* __restrict__ plane, int h, int w, NiqeWindow win,
                                                          double* __restrict__ stats) {
#pragma clang fp contract(off)
    constexpr int PW = BS + 6;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* patch = reinterpret_cast<float*>(smem);
    float* nn = patch + PW * PW;
    __shared__ double red[NQ_T / 64][25];
    const int t = threadIdx.x, bx = blockIdx.x, by = blockIdx.y, smp = blockIdx.z;
    const float* src = plane + (size_t)smp * h * w;
    for (int i = t; i < PW * PW; i += NQ_T) {
        const int py = i / PW, px = i - py * PW;
        const int gy = min(max(by * BS - 3 + py, 0), h - 1), gx = min(max(bx * BS - 3 + px, 0), w - 1);
        patch[i] = src[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int i = t; i < BS * BS; i += NQ_T) {
        const int y = i / BS, x = i - y * BS;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
#pragma unroll
            for (int b = 0; b < 7; ++b) {
                const float p = patch[(y + a) * PW + x + b];
                const float q = p * p;                       // np.square of the float32 image
                const double wk = win.w[a * 7 + b];
                a1 = a1 + wk * (double)p;
                a2 = a2 + wk * (double)q;
            }
        }
        const float mu = (float)a1, m2 = (float)a2;          // scipy rounds its double sums to the float32 output
        const float musq = mu * mu;
        const float var = m2 - musq;
        const float sigma = __builtin_sqrtf(__builtin_fabsf(var));
        const float c = patch[(y + 3) * PW + x + 3];
        const float num = c - mu, den = sigma + 1.0f;
        nn[i] = num / den;
    }
    __syncthreads();
    double acc[25];
#pragma unroll
    for (int q = 0; q < 25; ++q) acc[q] = 0.0;
    for (int i = t; i < BS * BS; i += NQ_T) {
        const int y = i / BS, x = i - y * BS;
        const int ym = y == 0 ? BS - 1 : y - 1, xm = x == 0 ? BS - 1 : x - 1, xp = x == BS - 1 ? 0 : x + 1;
        const float v = nn[i];
        // np.roll(n, s)[y][x] = n[y - s0][x - s1], wrapped inside the block: s = (0,1), (1,0), (1,1), (1,-1)
        const float maps[5] = {v, v * nn[y * BS + xm], v * nn[ym * BS + x], v * nn[ym * BS + xm], v * nn[ym * BS + xp]};
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const float u = maps[m];
            const float sq = u * u;                          // the square is a float32, as block ** 2 is
            const bool neg = u < 0.f, pos = u > 0.f;
            acc[5 * m + 0] += neg ? 1.0 : 0.0;
            acc[5 * m + 1] += pos ? 1.0 : 0.0;
            acc[5 * m + 2] += neg ? (double)sq : 0.0;
            acc[5 * m + 3] += pos ? (double)sq : 0.0;
            acc[5 * m + 4] += (double)__builtin_fabsf(u);
        }
    }
    // fixed order: a shuffle tree inside each wave, then the four waves in order
#pragma unroll
    for (int q = 0; q < 25; ++q) {
        double s = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((t & 63) == 0) red[t >> 6][q] = s;
    }
    __syncthreads();
    if (t < 25) {
        const double s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        stats[(((size_t)smp * gridDim.y + by) * gridDim.x + bx) * 25 + t] = s;
    }
}

struct NiqeGeom {
    int H, W;   // the block-cropped plane
};

int niqe_geometry(int32_t B, int32_t h, int32_t w, int32_t crop, NiqeGeom* g) {
    if (B < 1 || h < 1 || w < 1 || crop < 0 || B > 65535) return HAT_EINVAL;
    const int64_t hc = (int64_t)h - 2 * (int64_t)crop, wc = (int64_t)w - 2 * (int64_t)crop;
    if (hc < NQ_BLOCK || wc < NQ_BLOCK) return HAT_EINVAL;   // no whole block is left
    g->H = (int)(hc / NQ_BLOCK) * NQ_BLOCK;
    g->W = (int)(wc / NQ_BLOCK) * NQ_BLOCK;
    if (g->H > 65535) return HAT_EINVAL;                      // the grid
    return 0;
}

template <int BS> int launch_blocks(const float* plane, int B, int h, int w, const NiqeWindow& win, double* stats, hipStream_t st) {
    constexpr int lds = ((BS + 6) * (BS + 6) + BS * BS) * 4;
    static_assert(lds + 1024 <= HAT_LDS_MAX, "the patch and n must fit in LDS");
    auto kern = niqe_block_kernel<BS>;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    HAT_LAUNCH(kern, dim3(w / BS, h / BS, B), dim3(NQ_T), lds, st, plane, h, w, win, stats);
    return hat_check_launch();
}

}  // namespace

extern "C" int hat_niqe_workspace_bytes(int32_t B, int32_t h, int32_t w, int32_t crop_border, int32_t* H96, int32_t* W96, int64_t* bytes) {
    NiqeGeom g;
    if (!H96 || !W96 || !bytes) return HAT_EINVAL;
    if (int rc = niqe_geometry(B, h, w, crop_border, &g)) return rc;
    *H96 = g.H;
    *W96 = g.W;
    // plane, its / 255 copy, the H pass's intermediate (H / 2 x W) and the half-size plane, fp32
    const int64_t px = (int64_t)g.H * g.W;
    *bytes = (int64_t)B * 4 * (px + px + px / 2 + px / 4);
    return 0;
}

extern "C" int hat_niqe_y_u8(const uint8_t* src, int64_t pitch, int64_t bstride, int32_t B, int32_t h, int32_t w, int32_t crop_border,
                             int32_t bgr, float* plane, float* unit, void* stream) {
    NiqeGeom g;
    if (!src || !plane) return HAT_EINVAL;
    if (int rc = niqe_geometry(B, h, w, crop_border, &g)) return rc;
    const int64_t row = 3 * (int64_t)w;
    if (pitch < row || (B > 1 && bstride < pitch * (int64_t)(h - 1) + row)) return HAT_EINVAL;
    HAT_LAUNCH(niqe_y_kernel, dim3((g.W + NQ_T - 1) / NQ_T, g.H, B), dim3(NQ_T), 0, reinterpret_cast<hipStream_t>(stream), src,
               (long long)pitch, (long long)bstride, (int)crop_border, g.H, g.W, bgr ? 1 : 0, plane, unit);
    return hat_check_launch();
}

extern "C" int hat_imresize_plane_rows(const float* src, float* mid, int32_t B, int32_t h, int32_t w, int32_t oh, const float* w_h,
                                       const int32_t* src_h, int32_t P_h, int64_t n_table, void* stream) {
    if (!src || !mid || !w_h || !src_h || B < 1 || h < 1 || w < 1 || oh < 1 || P_h < 1 || B > 65535 || oh > 65535) return HAT_EINVAL;
    if (n_table != (int64_t)oh * P_h) return HAT_EINVAL;
    HAT_LAUNCH(plane_rows_kernel, dim3((w + NQ_T - 1) / NQ_T, oh, B), dim3(NQ_T), 0, reinterpret_cast<hipStream_t>(stream), src, mid, w_h,
               src_h, (int)P_h, h, w, oh);
    return hat_check_launch();
}

extern "C" int hat_imresize_plane_cols(const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w,
                                       const int32_t* src_w, int32_t P_w, int64_t n_table, float out_scale, float* dst, void* stream) {
    if (!mid || !dst || !w_w || !src_w || B < 1 || oh < 1 || w < 1 || ow < 1 || P_w < 1 || B > 65535 || oh > 65535) return HAT_EINVAL;
    if (n_table != (int64_t)ow * P_w) return HAT_EINVAL;
    HAT_LAUNCH(plane_cols_kernel, dim3((ow + NQ_T - 1) / NQ_T, oh, B), dim3(NQ_T), 0, reinterpret_cast<hipStream_t>(stream), mid, w, oh, ow,
               w_w, src_w, (int)P_w, out_scale, dst);
    return hat_check_launch();
}

extern "C" int hat_niqe_block_stats(const float* plane, int32_t B, int32_t h, int32_t w, int32_t block, const double* window,
                                    double* stats, void* stream) {
    if (!plane || !window || !stats || B < 1 || B > 65535) return HAT_EINVAL;
    if (block != NQ_BLOCK && block != NQ_BLOCK / 2) return HAT_EINVAL;
    if (h < block || w < block || h % block || w % block || h / block > 65535) return HAT_EINVAL;
    NiqeWindow win;
    for (int i = 0; i < 49; ++i) win.w[i] = window[i];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return block == NQ_BLOCK ? launch_blocks<NQ_BLOCK>(plane, B, h, w, win, stats, st) : launch_blocks<NQ_BLOCK / 2>(plane, B, h, w, win, stats, st);
}
