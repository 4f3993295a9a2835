// hat_naf.hip — the NAFNet-style stem of HybridHATNAF (hybrid_hat_naf_arch.py:16-82) on gfx950.
//
// The global pool of a NAFBlock (its SCA) splits the block into two halves of one shape: 1x1 c -> 2c, depthwise 3x3, gate.
//   hat_naf_half  one half for one 8 x 16 pixel tile with a 1-pixel halo; the residual-stream row it starts from is either
//                 loaded (form a) or formed as r + Wf . gprev + bf from the previous half's gated map (form b)
//   hat_naf_fold  per sample: pool partials -> mean -> s = Wsca . mean + bsca -> Wf = beta * W2 * diag(s), bf = beta * b2
// Contracts: include/hat_mi355x.h "NAF stem".  DESIGN.md 4.13.
#include "hat_common.h"

namespace {

constexpr int NAF_TH = 8, NAF_TW = 16;                   // own pixels of a tile
constexpr int NAF_HH = NAF_TH + 2, NAF_HW = NAF_TW + 2;  // with the depthwise conv's halo
constexpr int NAF_HPX = NAF_HH * NAF_HW;                 // 180 halo pixels ...
constexpr int NAF_PT = (NAF_HPX + 15) / 16;              // ... in 12 MFMA pixel tiles
constexpr int NAF_NPX = NAF_PT * 16;                     // 192 rows of every LDS image (rows >= 180 hold zeros)
constexpr int NAF_THREADS = 256;

template <typename T, int C> struct NafLds {
    static constexpr int LDX = lds_row_elems(C, sizeof(T));   // MFMA operand rows (T)
    static constexpr int LDU = 2 * C + 4;                     // u rows (fp32)
    static constexpr size_t US = (size_t)NAF_NPX * LDU * sizeof(float);
    static constexpr size_t XS = (size_t)NAF_NPX * LDX * sizeof(T);
    static constexpr size_t BYTES = US + XS;
    static_assert(XS <= US, "the staged gated map aliases the u image");
    static_assert((size_t)(NAF_THREADS / (C / 4)) * C * sizeof(float) <= XS, "the pool's partial rows alias the operand image");
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

// LDS: [ us: u = W1 r + b1, fp32 [192][LDU]  (form b first stages gprev here as T [192][LDX]) | rs: r as T [192][LDX] ]
// Every wave keeps the A fragments of the output-channel tiles it owns in registers for the whole workgroup.
template <typename T, int C>
__global__ __launch_bounds__(NAF_THREADS) void naf_half_kernel(const HatNafHalfDesc d, const int tiles_x) {
    typedef NafLds<T, C> L;
    typedef typename MT<T>::frag_t frag_t;
    constexpr int KS = C / 32, LDX = L::LDX, LDU = L::LDU;
    extern __shared__ __attribute__((aligned(16))) unsigned char naf_smem[];
    float* us = reinterpret_cast<float*>(naf_smem);
    T* gs = reinterpret_cast<T*>(naf_smem);
    T* rs = reinterpret_cast<T*>(naf_smem + L::US);
    float* red = reinterpret_cast<float*>(naf_smem + L::US);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int ty0 = (tile / tiles_x) * NAF_TH, tx0 = (tile % tiles_x) * NAF_TW;
    const int H = d.H, W = d.W;
    const int64_t pix0 = (int64_t)b * H * W;

    // halo pixel p -> its pixel index in the sample's map, or -1 outside the image (and for the pad rows p >= 180)
    auto pixel = [&](int p) -> int64_t {
        const int yy = ty0 - 1 + p / NAF_HW, xx = tx0 - 1 + p % NAF_HW;
        return (p < NAF_HPX && yy >= 0 && yy < H && xx >= 0 && xx < W) ? pix0 + (int64_t)yy * W + xx : -1;
    };
    auto own = [&](int p) -> bool {
        const int hy = p / NAF_HW, hx = p % NAF_HW;
        return hy >= 1 && hy <= NAF_TH && hx >= 1 && hx <= NAF_TW;
    };

    if (d.gprev) {
        // ---- form (b): r = r_in + Wf . gprev + bf on every halo pixel; written out for the tile's own pixels
        constexpr int VEC = MT<T>::VEC, PV = C / VEC;
        const T* gp = reinterpret_cast<const T*>(d.gprev);
        for (int i = tid; i < NAF_NPX * PV; i += NAF_THREADS) {
            const int p = i / PV, v = i % PV;
            const int64_t px = pixel(p);
            u32x4 val = {0u, 0u, 0u, 0u};
            if (px >= 0) val = *reinterpret_cast<const u32x4*>(gp + px * d.ldg + v * VEC);
            *reinterpret_cast<u32x4*>(gs + p * LDX + v * VEC) = val;
        }
        __syncthreads();
        constexpr int OT = C / 16;                   // 4 or 2 output-channel tiles over 4 waves
        const int ot = wave % OT;
        const T* wf = reinterpret_cast<const T*>(d.wf) + (int64_t)b * d.wf_bstride;
        frag_t a[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = MT<T>::load(wf + ((ot * KS + ks) * 64 + lane) * 8);
        const int ch = 16 * ot + 4 * g;
        const f32x4 bias = *reinterpret_cast<const f32x4*>(d.bf + (int64_t)b * d.bf_bstride + ch);
        for (int pt = wave / OT; pt < NAF_PT; pt += 4 / OT) {
            const int p = 16 * pt + l15;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = MT<T>::mma(a[ks], MT<T>::load(gs + p * LDX + 32 * ks + 8 * g), acc);
            const int64_t px = pixel(p);
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (px >= 0) {
                r = *reinterpret_cast<const f32x4*>(d.r_in + px * d.ldr + ch) + acc + bias;
                if (own(p)) *reinterpret_cast<f32x4*>(d.r_out + px * d.ldr + ch) = r;
            }
            Vec4<T>::store(rs + p * LDX + ch, r);
        }
        if (!d.w1) return;                           // projection only: the stream after the last block
    } else {
        // ---- form (a): the stored stream
        constexpr int PV = C / 4;
        for (int i = tid; i < NAF_NPX * PV; i += NAF_THREADS) {
            const int p = i / PV, v = i % PV;
            const int64_t px = pixel(p);
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (px >= 0) r = *reinterpret_cast<const f32x4*>(d.r_in + px * d.ldr + 4 * v);
            Vec4<T>::store(rs + p * LDX + 4 * v, r);
        }
    }
    __syncthreads();   // rs is complete; nobody reads gs any more

    // ---- u = W1 . r + b1 on the MFMA units; u = 0 (not b1) where the pixel lies outside the image: the depthwise conv pads u
    {
        constexpr int OT2 = 2 * C / 16;
        const T* w1 = reinterpret_cast<const T*>(d.w1);
        for (int ot = wave; ot < OT2; ot += 4) {
            frag_t a[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[ks] = MT<T>::load(w1 + ((ot * KS + ks) * 64 + lane) * 8);
            const int ch = 16 * ot + 4 * g;
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(d.b1 + ch);
            for (int pt = 0; pt < NAF_PT; ++pt) {
                const int p = 16 * pt + l15;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = MT<T>::mma(a[ks], MT<T>::load(rs + p * LDX + 32 * ks + 8 * g), acc);
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(us + p * LDU + ch) = pixel(p) >= 0 ? acc + b1 : zero;
            }
        }
    }
    __syncthreads();   // us is complete; nobody reads rs any more

    // ---- depthwise 3x3 + bias on both channel halves, gate, store; a thread keeps one group of 4 channels for all its pixels
    constexpr int CG = C / 4;
    const int c0 = 4 * (tid % CG);
    f32x4 wa[9], wb[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        wa[t] = *reinterpret_cast<const f32x4*>(d.dww + t * 2 * C + c0);
        wb[t] = *reinterpret_cast<const f32x4*>(d.dww + t * 2 * C + C + c0);
    }
    const f32x4 ba = *reinterpret_cast<const f32x4*>(d.dwb + c0), bb = *reinterpret_cast<const f32x4*>(d.dwb + C + c0);
    T* gout = reinterpret_cast<T*>(d.g_out);
    f32x4 psum = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < NAF_TH * NAF_TW * CG; i += NAF_THREADS) {
        const int pxi = i / CG, oy = pxi / NAF_TW, ox = pxi % NAF_TW;
        const int yy = ty0 + oy, xx = tx0 + ox;
        if (yy >= H || xx >= W) continue;
        f32x4 va = ba, vb = bb;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float* up = us + ((oy + t / 3) * NAF_HW + ox + t % 3) * LDU;
            va += wa[t] * *reinterpret_cast<const f32x4*>(up + c0);
            vb += wb[t] * *reinterpret_cast<const f32x4*>(up + C + c0);
        }
        const f32x4 gq = va * vb;
        Vec4<T>::store(gout + (pix0 + (int64_t)yy * W + xx) * d.ldo + c0, gq);
        psum += gq;
    }

    // ---- the pool's share of this tile: fp32 values before rounding, summed in a fixed order, one slot per tile
    if (d.partials) {
        constexpr int ROWS = NAF_THREADS / CG;
        *reinterpret_cast<f32x4*>(red + (tid / CG) * C + c0) = psum;
        __syncthreads();
        if (tid < C) {
            float s = 0.f;
            for (int r = 0; r < ROWS; ++r) s += red[r * C + tid];
            d.partials[((int64_t)b * gridDim.x + tile) * C + tid] = s;
        }
    }
}

template <typename T, int C>
int naf_half_launch(const HatNafHalfDesc& d, hipStream_t s) {
    constexpr size_t lds = NafLds<T, C>::BYTES;
    auto kern = naf_half_kernel<T, C>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    // one workgroup per tile and sample, no persistent loop: 3600 workgroups per 720p sample cover the 256 CUs many times
    const int tiles_x = (d.W + NAF_TW - 1) / NAF_TW, tiles_y = (d.H + NAF_TH - 1) / NAF_TH;
    HAT_LAUNCH(kern, dim3(tiles_x * tiles_y, d.B), dim3(NAF_THREADS), lds, s, d, tiles_x);
    return hat_check_launch();
}

template <typename T, int C>
__global__ __launch_bounds__(NAF_THREADS) void naf_fold_kernel(const HatNafFoldDesc d) {
    constexpr int P = NAF_THREADS / C, KS = C / 32;
    __shared__ float part[NAF_THREADS];
    __shared__ float mean[C];
    __shared__ float sv[C];
    const int tid = threadIdx.x, b = blockIdx.x;
    {   // the pool: P strided partial sums per channel, then their sum, both in a fixed order
        const int c = tid % C, pr = tid / C;
        const float* pp = d.partials + (int64_t)b * d.tiles * C + c;
        float s = 0.f;
        for (int t = pr; t < d.tiles; t += P) s += pp[(int64_t)t * C];
        part[tid] = s;
    }
    __syncthreads();
    if (tid < C) {
        float m = 0.f;
        for (int r = 0; r < P; ++r) m += part[r * C + tid];
        mean[tid] = m / (float)d.npix;
    }
    __syncthreads();
    if (tid < C) {
        float a = d.bsca[tid];
        for (int i = 0; i < C; ++i) a = fmaf(d.wsca[tid * C + i], mean[i], a);
        sv[tid] = a;
        d.bf[(int64_t)b * C + tid] = d.beta[tid] * d.b2[tid];
    }
    __syncthreads();
    T* wf = reinterpret_cast<T*>(d.wf) + (int64_t)b * C * C;
    for (int idx = tid; idx < C * C; idx += NAF_THREADS) {   // fragment order [C/16][C/32][64 lanes][8]
        const int j = idx & 7, lane = (idx >> 3) & 63, rest = idx >> 9;
        const int o = 16 * (rest / KS) + (lane & 15), i = 32 * (rest % KS) + 8 * (lane >> 4) + j;
        wf[idx] = to_T<T>(d.beta[o] * d.w2[o * C + i] * sv[i]);
    }
}

template <typename T, int C>
int naf_fold_launch(const HatNafFoldDesc& d, hipStream_t s) {
    HAT_LAUNCH((naf_fold_kernel<T, C>), dim3(d.B), dim3(NAF_THREADS), 0, s, d);
    return hat_check_launch();
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

extern "C" int hat_naf_half_tiles(int32_t H, int32_t W) {
    if (H < 1 || W < 1) return HAT_EINVAL;
    return ((H + NAF_TH - 1) / NAF_TH) * ((W + NAF_TW - 1) / NAF_TW);
}

extern "C" int hat_naf_half(const HatNafHalfDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatNafHalfDesc& d = *dp;
    if (d.dtype != HAT_F32 && d.dtype != HAT_BF16) return HAT_EINVAL;
    if (d.B < 1 || d.B > 65535 || d.H < 1 || d.W < 1) return HAT_EINVAL;
    if (d.C != 64 && d.C != 32) return HAT_EUNSUPPORTED;
    const int vec = d.dtype == HAT_BF16 ? 8 : 4;
    if (!d.r_in || !aligned(d.r_in, 16) || d.ldr < d.C || d.ldr % 4) return HAT_EINVAL;
    if (d.gprev) {   // form (b)
        if (!d.wf || !d.bf || !d.r_out || d.r_out == d.r_in) return HAT_EINVAL;
        if (!aligned(d.gprev, 16) || !aligned(d.wf, 16) || !aligned(d.bf, 16) || !aligned(d.r_out, 16)) return HAT_EINVAL;
        if (d.ldg < d.C || d.ldg % vec || d.wf_bstride < 0 || d.wf_bstride % vec || d.bf_bstride < 0 || d.bf_bstride % 4) return HAT_EINVAL;
    } else if (!d.w1) {
        return HAT_EINVAL;   // nothing to do: form (a) with the c -> 2c stage switched off
    }
    if (d.w1) {
        if (!d.b1 || !d.dww || !d.dwb || !d.g_out || d.g_out == d.gprev) return HAT_EINVAL;
        if (!aligned(d.w1, 16) || !aligned(d.b1, 16) || !aligned(d.dww, 16) || !aligned(d.dwb, 16) || !aligned(d.g_out, 16)) return HAT_EINVAL;
        if (d.ldo < d.C || d.ldo % vec) return HAT_EINVAL;
    } else if (d.partials) {
        return HAT_EINVAL;   // no gated map, no pool
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.C == 64 ? naf_half_launch<bf16_t, 64>(d, s) : naf_half_launch<bf16_t, 32>(d, s);
    return d.C == 64 ? naf_half_launch<float, 64>(d, s) : naf_half_launch<float, 32>(d, s);
}

extern "C" int hat_naf_fold(const HatNafFoldDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatNafFoldDesc& d = *dp;
    if (d.dtype != HAT_F32 && d.dtype != HAT_BF16) return HAT_EINVAL;
    if (d.B < 1 || d.tiles < 1 || d.npix < 1) return HAT_EINVAL;
    if (d.C != 64 && d.C != 32) return HAT_EUNSUPPORTED;
    if (!d.partials || !d.wsca || !d.bsca || !d.w2 || !d.b2 || !d.beta || !d.wf || !d.bf) return HAT_EINVAL;
    if (!aligned(d.wf, 16) || !aligned(d.bf, 16)) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.C == 64 ? naf_fold_launch<bf16_t, 64>(d, s) : naf_fold_launch<bf16_t, 32>(d, s);
    return d.C == 64 ? naf_fold_launch<float, 64>(d, s) : naf_fold_launch<float, 32>(d, s);
}
