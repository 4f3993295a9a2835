// hat_escrealm.hip — what ESCRealM (esc_real_arch.py:478-661) adds to ESCReal's kernels, on gfx950.
//
//   hat_unshuffle_pad   check_img_size (reflect pad on the right and bottom to a multiple of f) and PixelUnshuffle(f) in one
//                       pass: x (B,3,h,w) fp32 planes -> rows (B, ceil(h/f), ceil(w/f), ld) fp32 with channel c f^2 + f i + j =
//                       x[c][refl(f yb + i)][refl(f xb + j)].  Both proj (hat_conv, HAT_X_NHWC_F32) and the skip branch read it.
//   hat_escrealm_skip   out = [r +] skip(rows), skip = 1x1 CIN -> 128, depthwise 7x7 with REFLECT padding, LeakyReLU(0.2),
//                       1x1 128 -> 64 for CIN = 12 or 48.  hat_escreal_skip folds the first two layers into one dense 7x7 conv
//                       (K = 49 * 3); at 12 or 48 channels that patch matrix no longer fits in LDS, so the layers stay apart:
//                       per 8 x 8 tile the 14 x 14 halo of the input rows goes to LDS (a 1x1 conv commutes with reflect padding:
//                       the halo is gathered at the mirrored pixels), the 128-wide hidden map of the halo is computed in fp32 and
//                       kept in LDS, the depthwise conv and the LeakyReLU run on it, and the last 1x1 is hat_escreal_skip's
//                       MFMA stage.  Nothing 128 wide reaches HBM.
//   hat_shuffle_planes  y[b][c][s yy + i][s xx + j] = rows[b][yy][xx][c s^2 + s i + j]: hat_esc_shuffle_add without a base image.
// Contracts: include/hat_mi355x.h "ESCRealM".  DESIGN.md 4.18.
#include "hat_common.h"

namespace {

__global__ __launch_bounds__(256) void unshuffle_pad_kernel(const float* __restrict__ x, float* __restrict__ rows, int h, int w, int f,
                                                            int Hb, int Wb, int ld, int64_t total) {
    const int ff = f * f, cin = 3 * ff;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % cin);
        const int64_t px = i / cin;
        const int xb = (int)(px % Wb), yb = (int)((px / Wb) % Hb);
        const int64_t b = px / ((int64_t)Wb * Hb);
        const int c = ci / ff, ij = ci % ff;
        int yy = yb * f + ij / f, xx = xb * f + ij % f;
        yy = yy >= h ? 2 * h - 2 - yy : yy;   // (the pad is smaller than the side: one reflection lands inside)
        xx = xx >= w ? 2 * w - 2 - xx : xx;
        rows[px * ld + ci] = x[((b * 3 + c) * h + yy) * (int64_t)w + xx];
    }
}

__global__ __launch_bounds__(256) void shuffle_planes_kernel(const float* __restrict__ rows, float* __restrict__ y, int H, int W, int s, int ld,
                                                             int64_t total) {
    const int Hs = H * s, Ws = W * s;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % Ws), Y = (int)((i / Ws) % Hs), c = (int)((i / ((int64_t)Ws * Hs)) % 3);
        const int64_t b = i / ((int64_t)Ws * Hs * 3);
        const int64_t px = (b * H + Y / s) * W + X / s;
        y[i] = rows[px * ld + c * s * s + (Y % s) * s + X % s];
    }
}

// ---------------------------------------------------------------------------------------------
// the skip branch over 12 or 48 input channels
// ---------------------------------------------------------------------------------------------
constexpr int EMS_C = 64, EMS_HID = 128, EMS_T = 8, EMS_PX = EMS_T * EMS_T, EMS_HW = EMS_T + 6, EMS_HP = EMS_HW * EMS_HW, EMS_THREADS = 256;

template <typename T, int CIN> struct EmsLds {
    static constexpr int LDH = lds_row_elems(EMS_HID, sizeof(T));   // lrelu(depthwise) rows, MFMA operand
    static constexpr size_t XB = (size_t)EMS_HP * CIN * sizeof(float), HB = (size_t)EMS_PX * LDH * sizeof(T);
    static constexpr size_t XS = ((XB > HB ? XB : HB) + 15) / 16 * 16;   // the input halo, then (dead by then) the hidden rows
    static constexpr size_t BYTES = XS + (size_t)EMS_HP * EMS_HID * sizeof(float);
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

struct EmsArgs {
    const float* x; const float* w0; const float* b0; const float* dw; const float* bdw; const void* w3; const float* b3; const float* r;
    float* out;
    int H, W, tiles_x, ldx, ldr, ldo;
};

// LDS: [ xs: the 14x14 halo of the input rows, fp32 [196][CIN]; reused as hs: lrelu(depthwise) as T [64][LDH] | hid: fp32 [196][128] ]
template <typename T, int CIN>
__global__ __launch_bounds__(EMS_THREADS) void escrealm_skip_kernel(const EmsArgs a) {
    typedef EmsLds<T, CIN> L;
    typedef typename MT<T>::frag_t frag_t;
    constexpr int KS2 = EMS_HID / 32, LDH = L::LDH, PT = EMS_PX / 16, Q = CIN / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char ems_smem[];
    float* xs = reinterpret_cast<float*>(ems_smem);
    T* hs = reinterpret_cast<T*>(ems_smem);
    float* hid = reinterpret_cast<float*>(ems_smem + L::XS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int H = a.H, W = a.W, b = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / a.tiles_x) * EMS_T, tx0 = (int)(blockIdx.x % a.tiles_x) * EMS_T;
    const int64_t n = (int64_t)H * W;
    const float* xb = a.x + (int64_t)b * n * a.ldx;

    // ---- halo: a position past an edge reads the pixel it mirrors (H, W >= 4); the halo of pixels past the frame (a partial
    //      tile; computed and dropped) is clamped so that every read stays inside
    for (int i = tid; i < EMS_HP * Q; i += EMS_THREADS) {
        const int p = i / Q, q = i % Q;
        int yy = ty0 + p / EMS_HW - 3, xx = tx0 + p % EMS_HW - 3;
        yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
        xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
        yy = min(max(yy, 0), H - 1);
        xx = min(max(xx, 0), W - 1);
        *reinterpret_cast<f32x4*>(xs + p * CIN + 4 * q) = *reinterpret_cast<const f32x4*>(xb + ((int64_t)yy * W + xx) * a.ldx + 4 * q);
    }
    __syncthreads();

    // ---- hidden = W0 . x + b0 over the halo, fp32; thread = (channel, every other position)
    const int c = tid & (EMS_HID - 1), half = tid >> 7;
    {
        float w0[CIN];
#pragma unroll
        for (int k = 0; k < CIN; ++k) w0[k] = a.w0[c * CIN + k];
        const float b0 = a.b0[c];
        for (int p = half; p < EMS_HP; p += 2) {
            float acc = b0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xs + p * CIN + 4 * q);
                acc += w0[4 * q] * v[0] + w0[4 * q + 1] * v[1] + w0[4 * q + 2] * v[2] + w0[4 * q + 3] * v[3];
            }
            hid[p * EMS_HID + c] = acc;
        }
    }
    __syncthreads();

    // ---- hs = lrelu_0.2(depthwise 7x7 + bdw); thread = (channel, 32 pixels)
    {
        float dw[49];
#pragma unroll
        for (int k = 0; k < 49; ++k) dw[k] = a.dw[c * 49 + k];
        const float bdw = a.bdw[c];
        for (int p = half * (EMS_PX / 2); p < (half + 1) * (EMS_PX / 2); ++p) {
            const float* hp = hid + ((p / EMS_T) * EMS_HW + p % EMS_T) * EMS_HID + c;
            float acc = bdw;
#pragma unroll
            for (int k = 0; k < 49; ++k) acc += dw[k] * hp[((k / 7) * EMS_HW + k % 7) * EMS_HID];
            hs[p * LDH + c] = to_T<T>(acc >= 0.f ? acc : 0.2f * acc);
        }
    }
    __syncthreads();

    // ---- out = W3 . hidden + b3 [+ r]; wave w owns output channels 16 w .. 16 w + 15
    {
        const T* w3 = reinterpret_cast<const T*>(a.w3);
        frag_t af[KS2];
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) af[ks] = MT<T>::load(w3 + ((wave * KS2 + ks) * 64 + lane) * 8);
        const int ch = 16 * wave + 4 * g;
        const f32x4 b3 = *reinterpret_cast<const f32x4*>(a.b3 + ch);
        for (int pt = 0; pt < PT; ++pt) {
            const int p = 16 * pt + l15;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) acc = MT<T>::mma(af[ks], MT<T>::load(hs + p * LDH + 32 * ks + 8 * g), acc);
            const int y = ty0 + p / EMS_T, x = tx0 + p % EMS_T;
            if (y < H && x < W) {
                const int64_t px = (int64_t)b * n + (int64_t)y * W + x;
                f32x4 v = acc + b3;
                if (a.r) v += *reinterpret_cast<const f32x4*>(a.r + px * a.ldr + ch);
                *reinterpret_cast<f32x4*>(a.out + px * a.ldo + ch) = v;
            }
        }
    }
}

template <typename T, int CIN>
int escrealm_skip_launch(const EmsArgs& a, int B, int tiles, hipStream_t s) {
    constexpr size_t lds = EmsLds<T, CIN>::BYTES;
    auto kern = escrealm_skip_kernel<T, CIN>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    HAT_LAUNCH(kern, dim3((unsigned)tiles, B), dim3(EMS_THREADS), lds, s, a);
    return hat_check_launch();
}

bool aligned(const void* p, uintptr_t al) { return reinterpret_cast<uintptr_t>(p) % al == 0; }

}  // namespace

extern "C" int hat_unshuffle_pad(const float* x, float* rows, int32_t B, int32_t h, int32_t w, int32_t f, int32_t ld, void* stream) {
    if (!x || !rows || B < 1 || h < 1 || w < 1) return HAT_EINVAL;
    if (f != 2 && f != 4) return HAT_EUNSUPPORTED;
    if (!aligned(x, 4) || !aligned(rows, 4) || ld < 3 * f * f) return HAT_EINVAL;
    if (h > 0x7fffffff - f || w > 0x7fffffff - f) return HAT_EINVAL;
    if ((f - h % f) % f > h - 1 || (f - w % f) % f > w - 1) return HAT_EINVAL;   // a reflect pad must be smaller than the side
    if (reinterpret_cast<const void*>(x) == reinterpret_cast<const void*>(rows)) return HAT_EINVAL;
    const int Hb = (h + f - 1) / f, Wb = (w + f - 1) / f;
    const int64_t total = (int64_t)B * Hb * Wb * 3 * f * f;
    const int64_t blocks = (total + 255) / 256;
    // tests/test_gpu_escreal_edges.py: UNSHUF_TRIP_VALUES = 8192 * 256 row values per trip
    HAT_LAUNCH(unshuffle_pad_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, rows,
               h, w, f, Hb, Wb, ld, total);
    return hat_check_launch();
}

extern "C" int hat_shuffle_planes(const float* rows, float* y, int32_t B, int32_t H, int32_t W, int32_t s, int32_t ld, void* stream) {
    if (!rows || !y || B < 1 || H < 1 || W < 1 || s < 1 || s > 8 || ld < 3 * s * s) return HAT_EINVAL;
    if (!aligned(rows, 4) || !aligned(y, 4) || reinterpret_cast<const void*>(rows) == reinterpret_cast<const void*>(y)) return HAT_EINVAL;
    if ((int64_t)H * s > 0x7fffffff / ((int64_t)W * s)) return HAT_EINVAL;   // a plane's pixel count fits an int
    const int64_t total = (int64_t)B * 3 * H * s * W * s;
    const int64_t blocks = (total + 255) / 256;
    // tests/test_gpu_escreal_edges.py: SHUFP_TRIP_OUTPUTS = 8192 * 256 output values per trip
    HAT_LAUNCH(shuffle_planes_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows, y,
               H, W, s, ld, total);
    return hat_check_launch();
}

extern "C" int hat_escrealm_skip(const float* x, const float* w0, const float* b0, const float* dw, const float* bdw, const void* w3,
                                 const float* b3, const float* r, float* out, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t ldx,
                                 int32_t ldr, int32_t ldo, int32_t dtype, void* stream) {
    if (!x || !w0 || !b0 || !dw || !bdw || !w3 || !b3 || !out) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (cin != 12 && cin != 48) return HAT_EUNSUPPORTED;
    if (B < 1 || B > 65535 || H < 4 || W < 4) return HAT_EINVAL;   // reflect pad 3 needs a side of at least 4
    const int64_t tiles = (int64_t)((H + EMS_T - 1) / EMS_T) * ((W + EMS_T - 1) / EMS_T);
    if (tiles > 0x7fffffff) return HAT_EINVAL;
    if (!aligned(x, 16) || !aligned(w0, 4) || !aligned(b0, 4) || !aligned(dw, 4) || !aligned(bdw, 4) || !aligned(w3, 16) || !aligned(b3, 16) ||
        !aligned(out, 16))
        return HAT_EINVAL;
    if (ldx < cin || ldx % 4 || ldo < EMS_C || ldo % 4) return HAT_EINVAL;
    if (r && (!aligned(r, 16) || ldr < EMS_C || ldr % 4)) return HAT_EINVAL;
    if (reinterpret_cast<const void*>(out) == reinterpret_cast<const void*>(x)) return HAT_EINVAL;
    const EmsArgs a{x, w0, b0, dw, bdw, w3, b3, r, out, H, W, (W + EMS_T - 1) / EMS_T, ldx, ldr, ldo};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == HAT_BF16)
        return cin == 12 ? escrealm_skip_launch<bf16_t, 12>(a, B, (int)tiles, s) : escrealm_skip_launch<bf16_t, 48>(a, B, (int)tiles, s);
    return cin == 12 ? escrealm_skip_launch<float, 12>(a, B, (int)tiles, s) : escrealm_skip_launch<float, 48>(a, B, (int)tiles, s);
}
