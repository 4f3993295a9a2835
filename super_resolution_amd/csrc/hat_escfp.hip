// hat_escfp.hip — what the ESCFP network (esc_fp_arch.py:247-355) adds to ESC's kernels, on gfx950.
//
//   hat_escfp_convffn           the ConvFFN of hat_esc_ffn.h at 48 channels (hidden 60 -> 64, 72 / 96 -> 96)
//   hat_escfp_layernorm         LayerNorm over 48 channels with eps as an argument
//   hat_escfp_weights           the per-sample weights of the DECOMPOSED large-kernel branch (esc_fp_arch.py:102-120) as the dense
//                               rank-1 filter hat_esc_conv13 / hat_conv read: pool -> 16 -> 4 -> GELU -> 144, K = lk_spatial + the
//                               dynamic 3x3 on the centre, weff[o][tap][i] = lk_channel[o][i] * K[o][tap]
//   hat_escfp_shuffle_bicubic   pixel_shuffle(to_img rows) + F.interpolate(x, scale_factor = s, mode = 'bicubic') -> fp32 planes
// Contracts: include/hat_mi355x.h "ESCFP".  DESIGN.md 4.16.
#include "hat_esc_ffn.h"

namespace {

constexpr int EFP_C = 48;
constexpr int EFP_PDIM = 16, EFP_K = 13, EFP_TAPS = EFP_K * EFP_K, EFP_HID = 4;
constexpr int EFW_THREADS = 1024, EFW_NP = EFW_THREADS / EFP_PDIM;   // 64 strided parts of the reduction

// One workgroup per (output channel co, sample b).
template <typename T>
__global__ __launch_bounds__(EFW_THREADS) void escfp_weights_kernel(const float* __restrict__ partials, int nblk, float inv_npix,
                                                                    const float* __restrict__ w1, const float* __restrict__ b1,
                                                                    const float* __restrict__ w2, const float* __restrict__ b2,
                                                                    const float* __restrict__ lk_channel, const float* __restrict__ lk_spatial,
                                                                    T* __restrict__ w_out, int Kpad) {
    __shared__ float part[EFW_THREADS];
    __shared__ float pmean[EFP_PDIM];
    __shared__ float hid[EFP_HID];
    __shared__ float kk[EFP_TAPS];
    const int tid = threadIdx.x, co = blockIdx.x, b = blockIdx.y;
    {   // fixed-order two-level reduction of the pool partials (esc_weights_kernel's discipline: no float atomics): 64 strided
        // parts, 8 independent chains each, the 8 loads of a trip unconditional (clamped + select) so that they are in flight together
        const int ci = tid & (EFP_PDIM - 1), pp = tid / EFP_PDIM;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* gp = partials + (size_t)b * nblk * EFP_PDIM + ci;
        for (int k0 = pp; k0 < nblk; k0 += EFW_NP * 8) {   // tests: one trip covers EFW_NP * 8 = 512 slots
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = gp[(size_t)min(k0 + EFW_NP * u, nblk - 1) * EFP_PDIM];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += (k0 + EFW_NP * u < nblk) ? v[u] : 0.f;
        }
        part[pp * EFP_PDIM + ci] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    __syncthreads();
    if (tid < EFP_PDIM) {
        float s = 0.f;
        for (int k = 0; k < EFW_NP; ++k) s += part[k * EFP_PDIM + tid];
        pmean[tid] = s * inv_npix;
    }
    __syncthreads();
    if (tid < EFP_HID) {
        float s = b1[tid];
        for (int ci = 0; ci < EFP_PDIM; ++ci) s += w1[tid * EFP_PDIM + ci] * pmean[ci];
        hid[tid] = gelu_erf(s);
    }
    __syncthreads();
    if (tid < EFP_TAPS) {   // K[co] = lk_spatial[co] + the dynamic 3 x 3 padded by 5 (esc_fp_arch.py:107-117)
        const int dy = tid / EFP_K - EFP_K / 2, dx = tid % EFP_K - EFP_K / 2;
        float v = lk_spatial[co * EFP_TAPS + tid];
        if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) {
            const int t = co * 9 + (dy + 1) * 3 + (dx + 1);
            float s = b2[t];
            for (int m = 0; m < EFP_HID; ++m) s += w2[t * EFP_HID + m] * hid[m];
            v += s;
        }
        kk[tid] = v;
    }
    __syncthreads();
    // weff[co][16 tap + ci] = lk_channel[co][ci] * K[co][tap]: one fp32 product, rounded once to T; K past the 169 taps is zero
    T* dst = w_out + ((size_t)b * EFP_PDIM + co) * Kpad;
    for (int k = tid; k < Kpad; k += EFW_THREADS) {
        const int tap = k / EFP_PDIM, ci = k % EFP_PDIM;
        dst[k] = to_T<T>(tap < EFP_TAPS ? lk_channel[co * EFP_PDIM + ci] * kk[tap] : 0.f);
    }
}

// ptab [s][4]: the four Keys weights (A = -0.75) of output phase p, for the source taps first .. first + 3 with
// first = (2 p + 1 < s) ? -2 : -1 relative to the source pixel o / s; taps are clamped to the frame.
__global__ __launch_bounds__(256) void escfp_shuffle_bicubic_kernel(const float* __restrict__ rows, const float* __restrict__ x,
                                                                    const float* __restrict__ ptab, float* __restrict__ y, int H, int W, int s,
                                                                    int ld, int64_t total) {
    const int Hs = H * s, Ws = W * s;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % Ws), Y = (int)((i / Ws) % Hs), c = (int)((i / ((int64_t)Ws * Hs)) % 3);
        const int64_t b = i / ((int64_t)Ws * Hs * 3);
        const int yy = Y / s, xx = X / s, py = Y % s, px = X % s;
        const int y0 = yy + (2 * py + 1 < s ? -2 : -1), x0 = xx + (2 * px + 1 < s ? -2 : -1);
        const f32x4 wy = *reinterpret_cast<const f32x4*>(ptab + 4 * py), wx = *reinterpret_cast<const f32x4*>(ptab + 4 * px);
        const float* plane = x + (b * 3 + c) * (int64_t)H * W;
        int xi[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) xi[t] = min(max(x0 + t, 0), W - 1);
        float base = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* row = plane + (int64_t)min(max(y0 + a, 0), H - 1) * W;
            base += wy[a] * ((wx[0] * row[xi[0]] + wx[1] * row[xi[1]]) + (wx[2] * row[xi[2]] + wx[3] * row[xi[3]]));
        }
        y[i] = rows[((b * H + yy) * W + xx) * ld + c * s * s + py * s + px] + base;
    }
}

}  // namespace

extern "C" int hat_escfp_convffn(const HatEscConvFfnDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatEscConvFfnDesc& d = *dp;
    if (d.dtype != HAT_F32 && d.dtype != HAT_BF16) return HAT_EINVAL;
    if (d.B < 1 || d.B > 65535 || d.H < 1 || d.W < 1 || d.reserved0) return HAT_EINVAL;
    if (d.hid_p != 64 && d.hid_p != 96) return HAT_EUNSUPPORTED;
    if (const int e = esc_convffn_check(d, EFP_C)) return e;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.hid_p == 64 ? esc_convffn_launch<bf16_t, EFP_C, 64>(d, s) : esc_convffn_launch<bf16_t, EFP_C, 96>(d, s);
    return d.hid_p == 64 ? esc_convffn_launch<float, EFP_C, 64>(d, s) : esc_convffn_launch<float, EFP_C, 96>(d, s);
}

extern "C" int hat_escfp_layernorm(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx,
                                   int32_t ldy, int32_t dtype, void* stream) {
    return esc_layernorm_run<EFP_C>(x, y, gamma, beta, eps, npix, ldx, ldy, dtype, stream);
}

extern "C" int hat_escfp_weights(const float* partials, int32_t nblk, int64_t npix, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* lk_channel, const float* lk_spatial, void* w_out, int32_t B, int32_t Kpad,
                                 int32_t dtype, void* stream) {
    if (!partials || !w1 || !b1 || !w2 || !b2 || !lk_channel || !lk_spatial || !w_out) return HAT_EINVAL;
    if (B < 1 || B > 65535 || nblk < 1 || npix < 1 || Kpad < EFP_TAPS * EFP_PDIM) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(EFP_PDIM, B), block(EFW_THREADS);
    const float inv = 1.0f / (float)npix;
    if (dtype == HAT_BF16)
        HAT_LAUNCH(escfp_weights_kernel<bf16_t>, grid, block, 0, s, partials, nblk, inv, w1, b1, w2, b2, lk_channel, lk_spatial,
                   reinterpret_cast<bf16_t*>(w_out), Kpad);
    else if (dtype == HAT_F32)
        HAT_LAUNCH(escfp_weights_kernel<float>, grid, block, 0, s, partials, nblk, inv, w1, b1, w2, b2, lk_channel, lk_spatial,
                   reinterpret_cast<float*>(w_out), Kpad);
    else
        return HAT_EINVAL;
    return hat_check_launch();
}

extern "C" int hat_escfp_shuffle_bicubic(const float* rows, const float* x, const float* ptab, float* y, int32_t B, int32_t H, int32_t W,
                                         int32_t s, int32_t ld, void* stream) {
    if (!rows || !x || !ptab || !y || B < 1 || H < 1 || W < 1 || ld < 3 * s * s || !esc_aligned(ptab, 16)) return HAT_EINVAL;
    if (s < 2 || s > 4) return HAT_EUNSUPPORTED;
    const int64_t total = (int64_t)B * 3 * H * s * W * s;
    const int64_t blocks = (total + 255) / 256;
    // tests/test_gpu_escreal_edges.py: BICUBIC_TRIP_OUTPUTS = 8192 * 256 output values per trip
    HAT_LAUNCH(escfp_shuffle_bicubic_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
               rows, x, ptab, y, H, W, s, ld, total);
    return hat_check_launch();
}
