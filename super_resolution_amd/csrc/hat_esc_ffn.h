// hat_esc_ffn.h — the two kernels the ESC family shares across its widths, templated on the channel count C: the ConvFFN
// (hat_esc_convffn at C = 64 in hat_esc.hip, hat_escfp_convffn at C = 48 in hat_escfp.hip) and the LayerNorm with eps as an
// argument (hat_esc_layernorm / hat_escfp_layernorm).  Contracts: include/hat_mi355x.h "ESC" and "ESCFP".  DESIGN.md 4.14, 4.16.
//
// C = 48 is 1.5 MFMA k-steps: the x image in LDS and the W1 fragments are zero-padded to 64 columns (two full k-steps), 12 of a
// pixel's 16 lanes hold channels (the other four hold the pad and take part in the row sums with zeros), and three of the four
// waves own the output channels of the second GEMM.  At C = 64 every `own` below is true and the code is the one it was.
#pragma once
#include "hat_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// ConvFFN
// ---------------------------------------------------------------------------------------------
constexpr int ECF_TH = 8, ECF_TW = 12;                   // own pixels of a tile
constexpr int ECF_HH = ECF_TH + 2, ECF_HW = ECF_TW + 2;  // with the depthwise conv's halo
constexpr int ECF_HPX = ECF_HH * ECF_HW;                 // 140 halo pixels ...
constexpr int ECF_PT = (ECF_HPX + 15) / 16;              // ... in 9 MFMA pixel tiles
constexpr int ECF_NPX = ECF_PT * 16;                     // 144 rows of the halo images (rows >= 140 hold zeros)
constexpr int ECF_OPX = ECF_TH * ECF_TW;                 // 96 own pixels = 6 MFMA pixel tiles
constexpr int ECF_OPT = ECF_OPX / 16;
constexpr int ECF_THREADS = 256;
constexpr int ECF_POOL = 16;                             // channels of a pool partial slot

template <typename T, int C, int HIDP> struct EcfLds {
    static_assert(C % 16 == 0 && C <= 64, "a pixel's channels are held by at most 16 lanes, the outputs by at most 4 waves");
    static constexpr int CP = (C + 31) / 32 * 32;                 // x rows padded to whole k-steps
    static constexpr int LDX = lds_row_elems(CP, sizeof(T));      // x rows, MFMA operand (T)
    static constexpr int LDU = HIDP + 4;                          // h rows (fp32)
    static constexpr int LDH = lds_row_elems(HIDP, sizeof(T));    // h2 rows, MFMA operand (T)
    static constexpr size_t US = (size_t)ECF_NPX * LDU * sizeof(float);
    static constexpr size_t XS = (size_t)ECF_NPX * LDX * sizeof(T);
    static constexpr size_t HS = (size_t)ECF_OPX * LDH * sizeof(T);
    static constexpr size_t BYTES = US + (XS > HS ? XS : HS);     // the h2 image takes the x image's place
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

// LDS: [ us: h = gelu(W1 x + b1), fp32 [144][LDU] | xs: x (after the LayerNorm) as T [144][LDX], later hs: h2 as T [96][LDH] ]
template <typename T, int C, int HIDP>
__global__ __launch_bounds__(ECF_THREADS) void esc_convffn_kernel(const HatEscConvFfnDesc d, const int tiles_x) {
    typedef EcfLds<T, C, HIDP> L;
    typedef typename MT<T>::frag_t frag_t;
    constexpr int KS1 = L::CP / 32, KS2 = HIDP / 32, LDX = L::LDX, LDU = L::LDU, LDH = L::LDH;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecf_smem[];
    float* us = reinterpret_cast<float*>(ecf_smem);
    T* xs = reinterpret_cast<T*>(ecf_smem + L::US);
    T* hs = reinterpret_cast<T*>(ecf_smem + L::US);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int ty0 = (tile / tiles_x) * ECF_TH, tx0 = (tile % tiles_x) * ECF_TW;
    const int H = d.H, W = d.W;
    const int64_t pix0 = (int64_t)b * H * W;

    // halo pixel p -> its pixel index in the sample's map, or -1 outside the image (and for the pad rows p >= 140)
    auto pixel = [&](int p) -> int64_t {
        const int yy = ty0 - 1 + p / ECF_HW, xx = tx0 - 1 + p % ECF_HW;
        return (p < ECF_HPX && yy >= 0 && yy < H && xx >= 0 && xx < W) ? pix0 + (int64_t)yy * W + xx : -1;
    };

    // ---- x rows, 16 lanes (one DPP row) per pixel; the LayerNorm over the C channels is two row sums
    {
        const int v = tid & 15;
        const bool own = 4 * v < C;   // this lane holds four channels (else: four zero columns of the last k-step)
        f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
        if (d.ln_g && own) {
            gam = *reinterpret_cast<const f32x4*>(d.ln_g + 4 * v);
            bet = *reinterpret_cast<const f32x4*>(d.ln_b + 4 * v);
        }
        for (int p = tid >> 4; p < ECF_NPX; p += ECF_THREADS / 16) {   // 144 = 9 x 16: every lane runs every trip
            const int64_t px = pixel(p);
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (px >= 0 && own) r = *reinterpret_cast<const f32x4*>(d.x + px * d.ldx + 4 * v);
            if (d.ln_g) {
                const float mean = row_sum16((r[0] + r[1]) + (r[2] + r[3])) * (1.0f / C);
                f32x4 c = r - mean;
                if (!own) c = f32x4{0.f, 0.f, 0.f, 0.f};
                const float var = row_sum16((c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3])) * (1.0f / C);
                r = c * (1.0f / sqrtf(var + d.ln_eps)) * gam + bet;
            }
            Vec4<T>::store(xs + p * LDX + 4 * v, r);
        }
    }
    __syncthreads();

    // ---- h = gelu(W1 . x + b1) on the MFMA units; h = 0 where the pixel lies outside the image: the depthwise conv pads h
    {
        constexpr int OT1 = HIDP / 16;
        const T* w1 = reinterpret_cast<const T*>(d.w1);
        for (int ot = wave; ot < OT1; ot += 4) {
            frag_t a[KS1];
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) a[ks] = MT<T>::load(w1 + ((ot * KS1 + ks) * 64 + lane) * 8);
            const int ch = 16 * ot + 4 * g;
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(d.b1 + ch);
            for (int pt = 0; pt < ECF_PT; ++pt) {
                const int p = 16 * pt + l15;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) acc = MT<T>::mma(a[ks], MT<T>::load(xs + p * LDX + 32 * ks + 8 * g), acc);
                f32x4 hv = {0.f, 0.f, 0.f, 0.f};
                if (pixel(p) >= 0) {
                    acc += b1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) hv[r] = gelu_act<T>(acc[r]);
                }
                *reinterpret_cast<f32x4*>(us + p * LDU + ch) = hv;
            }
        }
    }
    __syncthreads();   // us is complete; nobody reads xs any more

    // ---- h2 = gelu(dw3x3(h) + bias) + h for the own pixels; a thread keeps one group of 4 hidden channels for all its pixels
    {
        constexpr int CG = HIDP / 4, ROWS = ECF_THREADS / CG, ACTIVE = ROWS * CG;
        if (tid < ACTIVE) {
            const int c0 = 4 * (tid % CG);
            f32x4 wt[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(d.dww + t * HIDP + c0);
            const f32x4 bd = *reinterpret_cast<const f32x4*>(d.dwb + c0);
            for (int pxi = tid / CG; pxi < ECF_OPX; pxi += ROWS) {
                const int oy = pxi / ECF_TW, ox = pxi % ECF_TW;
                f32x4 v = bd;
#pragma unroll
                for (int t = 0; t < 9; ++t) v += wt[t] * *reinterpret_cast<const f32x4*>(us + ((oy + t / 3) * ECF_HW + ox + t % 3) * LDU + c0);
                const f32x4 h = *reinterpret_cast<const f32x4*>(us + ((oy + 1) * ECF_HW + ox + 1) * LDU + c0);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = gelu_act<T>(v[r]) + h[r];
                Vec4<T>::store(hs + pxi * LDH + c0, v);
            }
        }
    }
    __syncthreads();

    // ---- out = W2 . h2 + b2 [+ r]; wave w owns output channels 16 w .. 16 w + 15 of every own pixel (C = 48: three waves)
    if (wave < C / 16) {
        const int ot = wave;
        const T* w2 = reinterpret_cast<const T*>(d.w2);
        frag_t a[KS2];
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) a[ks] = MT<T>::load(w2 + ((ot * KS2 + ks) * 64 + lane) * 8);
        const int ch = 16 * ot + 4 * g;
        const f32x4 b2 = *reinterpret_cast<const f32x4*>(d.b2 + ch);
        f32x4 psum = {0.f, 0.f, 0.f, 0.f};
        for (int pt = 0; pt < ECF_OPT; ++pt) {
            const int p = 16 * pt + l15;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) acc = MT<T>::mma(a[ks], MT<T>::load(hs + p * LDH + 32 * ks + 8 * g), acc);
            const int yy = ty0 + p / ECF_TW, xx = tx0 + p % ECF_TW;
            if (yy < H && xx < W) {
                const int64_t px = pix0 + (int64_t)yy * W + xx;
                f32x4 v = acc + b2;
                if (d.r) v += *reinterpret_cast<const f32x4*>(d.r + px * d.ldr + ch);
                if (d.out_f32) {
                    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(d.out) + px * d.ldo + ch) = v;
                    psum += v;
                } else {
                    Vec4<T>::store(reinterpret_cast<T*>(d.out) + px * d.ldo + ch, v);
                    psum += as_stored<T>(v);
                }
            }
        }
        // the pool's share of this tile: the stored values of channels 0..15, summed in a fixed order, one slot per tile
        if (d.partials && ot == 0) {   // (wave-uniform: all 64 lanes take part in the row sums)
            f32x4 s;
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] = row_sum16(psum[r]);
            if (l15 == 0) *reinterpret_cast<f32x4*>(d.partials + ((int64_t)b * gridDim.x + tile) * ECF_POOL + ch) = s;
        }
    }
}

template <typename T, int C, int HIDP>
int esc_convffn_launch(const HatEscConvFfnDesc& d, hipStream_t s) {
    constexpr size_t lds = EcfLds<T, C, HIDP>::BYTES;
    auto kern = esc_convffn_kernel<T, C, HIDP>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int tiles_x = (d.W + ECF_TW - 1) / ECF_TW, tiles_y = (d.H + ECF_TH - 1) / ECF_TH;
    HAT_LAUNCH(kern, dim3(tiles_x * tiles_y, d.B), dim3(ECF_THREADS), lds, s, d, tiles_x);
    return hat_check_launch();
}

inline bool esc_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// Everything hat_esc_convffn / hat_escfp_convffn refuse except the hidden width; C = the entry's channel count.
inline int esc_convffn_check(const HatEscConvFfnDesc& d, int C) {
    if (d.dtype != HAT_F32 && d.dtype != HAT_BF16) return HAT_EINVAL;
    if (d.B < 1 || d.B > 65535 || d.H < 1 || d.W < 1 || d.reserved0) return HAT_EINVAL;
    if (!d.x || !d.w1 || !d.b1 || !d.dww || !d.dwb || !d.w2 || !d.b2 || !d.out || d.out == d.x) return HAT_EINVAL;
    if (!esc_aligned(d.x, 16) || !esc_aligned(d.w1, 16) || !esc_aligned(d.b1, 16) || !esc_aligned(d.dww, 16) || !esc_aligned(d.dwb, 16)
        || !esc_aligned(d.w2, 16) || !esc_aligned(d.b2, 16) || !esc_aligned(d.out, 16)) return HAT_EINVAL;
    if (d.ldx < C || d.ldx % 4) return HAT_EINVAL;
    const int ovec = (d.dtype == HAT_BF16 && !d.out_f32) ? 8 : 4;
    if (d.ldo < C || d.ldo % ovec) return HAT_EINVAL;
    if ((d.ln_g == nullptr) != (d.ln_b == nullptr)) return HAT_EINVAL;
    if (d.ln_g && (!esc_aligned(d.ln_g, 16) || !esc_aligned(d.ln_b, 16) || !(d.ln_eps > 0.f))) return HAT_EINVAL;
    if (d.r && (!esc_aligned(d.r, 16) || d.ldr < C || d.ldr % 4)) return HAT_EINVAL;
    if (d.partials && !esc_aligned(d.partials, 16)) return HAT_EINVAL;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over C channels, eps as an argument
// ---------------------------------------------------------------------------------------------
template <typename T, int C>
__global__ __launch_bounds__(256) void esc_layernorm_kernel(const float* __restrict__ x, T* __restrict__ y, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int64_t npix, int ldx, int ldy) {
    const int v = threadIdx.x & 15;
    const bool own = 4 * v < C;   // C = 48: 12 of a pixel's 16 lanes hold channels, the others add zeros to the row sums
    f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
    if (own) {
        gam = *reinterpret_cast<const f32x4*>(gamma + 4 * v);
        bet = *reinterpret_cast<const f32x4*>(beta + 4 * v);
    }
    const int64_t trips = (npix + 15) / 16;   // 16 pixels per trip of a 256-thread group; every lane runs every trip of its group
    for (int64_t t = (int64_t)blockIdx.x; t < trips; t += gridDim.x) {
        const int64_t px = 16 * t + (threadIdx.x >> 4);
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (px < npix && own) r = *reinterpret_cast<const f32x4*>(x + px * ldx + 4 * v);
        const float mean = row_sum16((r[0] + r[1]) + (r[2] + r[3])) * (1.0f / C);
        f32x4 c = r - mean;
        if (!own) c = f32x4{0.f, 0.f, 0.f, 0.f};
        const float var = row_sum16((c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3])) * (1.0f / C);
        r = c * (1.0f / sqrtf(var + eps)) * gam + bet;
        if (px < npix && own) Vec4<T>::store(y + px * ldy + 4 * v, r);
    }
}

constexpr int ESC_LN_MAX_GRID = 4096;   // tests: a pixel count above 16 * 4096 takes several grid trips

template <int C>
int esc_layernorm_run(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx, int32_t ldy,
                      int32_t dtype, void* stream) {
    if (!x || !y || !gamma || !beta || npix < 1 || !(eps > 0.f)) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (ldx < C || ldx % 4 || ldy < C || ldy % 4) return HAT_EINVAL;
    if (!esc_aligned(x, 16) || !esc_aligned(y, 8) || !esc_aligned(gamma, 16) || !esc_aligned(beta, 16)) return HAT_EINVAL;
    const int64_t trips = (npix + 15) / 16;
    const int grid = (int)(trips < ESC_LN_MAX_GRID ? trips : ESC_LN_MAX_GRID);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == HAT_BF16)
        HAT_LAUNCH((esc_layernorm_kernel<bf16_t, C>), dim3(grid), dim3(256), 0, s, x, reinterpret_cast<bf16_t*>(y), gamma, beta, eps, npix, ldx, ldy);
    else
        HAT_LAUNCH((esc_layernorm_kernel<float, C>), dim3(grid), dim3(256), 0, s, x, reinterpret_cast<float*>(y), gamma, beta, eps, npix, ldx, ldy);
    return hat_check_launch();
}

}  // namespace
