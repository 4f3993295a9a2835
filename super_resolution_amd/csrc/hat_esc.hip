// hat_esc.hip — what the ESC network (esc_arch.py:256-386) adds to the kernels its parts already have, on gfx950.
//
//   hat_esc_convffn           ConvFFN (esc_arch.py:148-159) for one 8 x 12 pixel tile with a 1-pixel halo, one launch:
//                             [LayerNorm eps] -> 1x1 64 -> hid -> GELU -> depthwise 3x3 -> GELU + h -> 1x1 hid -> 64 [+ residual],
//                             optionally with one deterministic pool partial per tile of the first 16 output channels
//   hat_window_attention_r    32 x 32 window attention (esc_arch.py:220-250), d = 16, all 1024 keys of a window-head in LDS;
//                             window positions past the frame read q, k, v at the reflected pixel (the 1x1 to_qkv commutes
//                             with the reflect pad) and their outputs are dropped
//   hat_esc_layernorm         LayerNorm over 64 channels with eps as an argument (esc_arch.py:68-86: 1e-6)
//   hat_esc_shuffle_add       pixel_shuffle(to_img rows + repeat_interleave(x, s*s)) (esc_arch.py:384-385) -> fp32 planes
// Contracts: include/hat_mi355x.h "ESC".  DESIGN.md 4.14.
#include "hat_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// ConvFFN
// ---------------------------------------------------------------------------------------------
constexpr int ECF_C = 64;
constexpr int ECF_TH = 8, ECF_TW = 12;                   // own pixels of a tile
constexpr int ECF_HH = ECF_TH + 2, ECF_HW = ECF_TW + 2;  // with the depthwise conv's halo
constexpr int ECF_HPX = ECF_HH * ECF_HW;                 // 140 halo pixels ...
constexpr int ECF_PT = (ECF_HPX + 15) / 16;              // ... in 9 MFMA pixel tiles
constexpr int ECF_NPX = ECF_PT * 16;                     // 144 rows of the halo images (rows >= 140 hold zeros)
constexpr int ECF_OPX = ECF_TH * ECF_TW;                 // 96 own pixels = 6 MFMA pixel tiles
constexpr int ECF_OPT = ECF_OPX / 16;
constexpr int ECF_THREADS = 256;
constexpr int ECF_POOL = 16;                             // channels of a pool partial slot

template <typename T, int HIDP> struct EcfLds {
    static constexpr int LDX = lds_row_elems(ECF_C, sizeof(T));   // x rows, MFMA operand (T)
    static constexpr int LDU = HIDP + 4;                          // h rows (fp32)
    static constexpr int LDH = lds_row_elems(HIDP, sizeof(T));    // h2 rows, MFMA operand (T)
    static constexpr size_t US = (size_t)ECF_NPX * LDU * sizeof(float);
    static constexpr size_t XS = (size_t)ECF_NPX * LDX * sizeof(T);
    static constexpr size_t HS = (size_t)ECF_OPX * LDH * sizeof(T);
    static constexpr size_t BYTES = US + (XS > HS ? XS : HS);     // the h2 image takes the x image's place
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

// LDS: [ us: h = gelu(W1 x + b1), fp32 [144][LDU] | xs: x (after the LayerNorm) as T [144][LDX], later hs: h2 as T [96][LDH] ]
template <typename T, int HIDP>
__global__ __launch_bounds__(ECF_THREADS) void esc_convffn_kernel(const HatEscConvFfnDesc d, const int tiles_x) {
    typedef EcfLds<T, HIDP> L;
    typedef typename MT<T>::frag_t frag_t;
    constexpr int C = ECF_C, KS1 = C / 32, KS2 = HIDP / 32, LDX = L::LDX, LDU = L::LDU, LDH = L::LDH;
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

    // ---- x rows, 16 lanes (one DPP row) per pixel; the LayerNorm over the 64 channels is two row sums
    {
        const int v = tid & 15;
        f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
        if (d.ln_g) {
            gam = *reinterpret_cast<const f32x4*>(d.ln_g + 4 * v);
            bet = *reinterpret_cast<const f32x4*>(d.ln_b + 4 * v);
        }
        for (int p = tid >> 4; p < ECF_NPX; p += ECF_THREADS / 16) {   // 144 = 9 x 16: every lane runs every trip
            const int64_t px = pixel(p);
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (px >= 0) r = *reinterpret_cast<const f32x4*>(d.x + px * d.ldx + 4 * v);
            if (d.ln_g) {
                const float mean = row_sum16((r[0] + r[1]) + (r[2] + r[3])) * (1.0f / C);
                const f32x4 c = r - mean;
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

    // ---- out = W2 . h2 + b2 [+ r]; wave w owns output channels 16 w .. 16 w + 15 of every own pixel
    {
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

template <typename T, int HIDP>
int esc_convffn_launch(const HatEscConvFfnDesc& d, hipStream_t s) {
    constexpr size_t lds = EcfLds<T, HIDP>::BYTES;
    auto kern = esc_convffn_kernel<T, HIDP>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int tiles_x = (d.W + ECF_TW - 1) / ECF_TW, tiles_y = (d.H + ECF_TH - 1) / ECF_TH;
    HAT_LAUNCH(kern, dim3(tiles_x * tiles_y, d.B), dim3(ECF_THREADS), lds, s, d, tiles_x);
    return hat_check_launch();
}

// ---------------------------------------------------------------------------------------------
// 32 x 32 window attention with reflected edges
// ---------------------------------------------------------------------------------------------
constexpr int WAR_WS = 32, WAR_N = WAR_WS * WAR_WS, WAR_D = 16, WAR_THREADS = 512;
constexpr int WAR_LDV = WAR_N + 4;                       // V^T rows: one channel's 1024 keys
constexpr int WAR_RPB = (2 * WAR_WS - 1) * (2 * WAR_WS - 1);   // 3969 bias entries per head
constexpr int WAR_RPB_PAD = (WAR_RPB + 3) / 4 * 4;

template <typename T> struct WarLds {
    static constexpr size_t KS = (size_t)WAR_N * WAR_D * sizeof(T);
    static constexpr size_t VS = (size_t)WAR_D * WAR_LDV * sizeof(T);
    static constexpr size_t BS = (size_t)WAR_RPB_PAD * sizeof(float);
    static constexpr size_t BYTES = KS + VS + BS;   // fp32: 64 + 64.25 + 15.5 KiB: K and V stay resident, no streaming
    static_assert(BYTES <= HAT_LDS_MAX, "K, V^T and the bias table do not fit in LDS");
};

template <typename T> __device__ __forceinline__ typename MT<T>::half_t war_p_frag(f32x4 p);
template <> __device__ __forceinline__ MT<float>::half_t war_p_frag<float>(f32x4 p) { return p; }
template <> __device__ __forceinline__ MT<bf16_t>::half_t war_p_frag<bf16_t>(f32x4 p) {
    typedef bf16_t v4 __attribute__((ext_vector_type(4)));
    const v4 h = {(bf16_t)p[0], (bf16_t)p[1], (bf16_t)p[2], (bf16_t)p[3]};
    return __builtin_bit_cast(MT<bf16_t>::half_t, h);
}

struct WarArgs {
    const void* q; const void* kv; const float* bias; void* out;
    int h, w, C, heads, nwx, ldq, ldkv, ldo;
};

// One workgroup = one (window, head).  S^T = K Q^T per 16 keys x 16 queries: in the MFMA D layout lane (query, g) then holds
// keys 4g .. 4g+3 — exactly the B operand of O^T = V^T P^T, so the probabilities never leave registers.  The relative-position
// bias is the C operand of the first MFMA.  Two passes over the keys: the row maximum, then exp / sum / P V.
template <typename T>
__global__ __launch_bounds__(WAR_THREADS) void window_attention_r_kernel(const WarArgs a) {
    typedef WarLds<T> L;
    typedef typename MT<T>::half_t half_t;
    constexpr int VEC = MT<T>::VEC, CV = WAR_D / VEC;
    extern __shared__ __attribute__((aligned(16))) unsigned char war_smem[];
    T* ks = reinterpret_cast<T*>(war_smem);
    T* vt = reinterpret_cast<T*>(war_smem + L::KS);
    float* bs = reinterpret_cast<float*>(war_smem + L::KS + L::VS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int head = blockIdx.x % a.heads, win = blockIdx.x / a.heads, b = blockIdx.y;
    const int y0 = (win / a.nwx) * WAR_WS, x0 = (win % a.nwx) * WAR_WS;
    const int h = a.h, w = a.w;
    // window position n -> the pixel that holds its q, k, v: itself, or its mirror image about the last row / column
    auto source = [&](int n) -> int64_t {
        int yy = y0 + (n >> 5), xx = x0 + (n & 31);
        if (yy >= h) yy = 2 * h - 2 - yy;
        if (xx >= w) xx = 2 * w - 2 - xx;
        return ((int64_t)b * h + yy) * w + xx;
    };

    const T* kvp = reinterpret_cast<const T*>(a.kv);
    for (int i = tid; i < WAR_N * CV; i += WAR_THREADS) {
        const int n = i / CV, c = (i % CV) * VEC;
        const T* src = kvp + source(n) * a.ldkv + head * WAR_D + c;
        *reinterpret_cast<u32x4*>(ks + n * WAR_D + c) = *reinterpret_cast<const u32x4*>(src);
        T tmp[VEC] __attribute__((aligned(16)));
        *reinterpret_cast<u32x4*>(tmp) = *reinterpret_cast<const u32x4*>(src + a.C);
#pragma unroll
        for (int e = 0; e < VEC; ++e) vt[(c + e) * WAR_LDV + n] = tmp[e];
    }
    for (int i = tid; i < WAR_RPB; i += WAR_THREADS) bs[i] = a.bias[(int64_t)head * WAR_RPB + i];
    __syncthreads();

    const T* qp = reinterpret_cast<const T*>(a.q);
    T* op = reinterpret_cast<T*>(a.out);
    for (int qg = wave; qg < WAR_N / 16; qg += WAR_THREADS / 64) {
        const int n = 16 * qg + l15, qy = n >> 5, qx = n & 31;
        const half_t qf = MT<T>::load_half(qp + source(n) * a.ldq + head * WAR_D + 4 * g);
        // logits of this lane's 4 keys of key tile kt: bias (key - query offsets) + k . q
        auto logits = [&](int kt) -> f32x4 {
            const float* bp = bs + ((kt >> 1) - qy + WAR_WS - 1) * (2 * WAR_WS - 1) + (16 * (kt & 1) + 4 * g - qx + WAR_WS - 1);
            const f32x4 acc = {bp[0], bp[1], bp[2], bp[3]};
            return MT<T>::mma_half(MT<T>::load_half(ks + (16 * kt + l15) * WAR_D + 4 * g), qf, acc);
        };
        float m = -INFINITY;
        for (int kt = 0; kt < WAR_N / 16; ++kt) {
            const f32x4 s = logits(kt);
            m = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < WAR_N / 16; ++kt) {
            f32x4 p = logits(kt);
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = expf(p[r] - m);
            l += (p[0] + p[1]) + (p[2] + p[3]);
            o = MT<T>::mma_half(MT<T>::load_half(vt + l15 * WAR_LDV + 16 * kt + 4 * g), war_p_frag<T>(p), o);
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const int yy = y0 + qy, xx = x0 + qx;
        if (yy < h && xx < w) Vec4<T>::store(op + (((int64_t)b * h + yy) * w + xx) * a.ldo + head * WAR_D + 4 * g, o * (1.0f / l));
    }
}

template <typename T>
int window_attention_r_launch(const WarArgs& a, int B, hipStream_t s) {
    constexpr size_t lds = WarLds<T>::BYTES;
    auto kern = window_attention_r_kernel<T>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    const int nwy = (a.h + WAR_WS - 1) / WAR_WS;
    HAT_LAUNCH(kern, dim3(a.nwx * nwy * a.heads, B), dim3(WAR_THREADS), lds, s, a);
    return hat_check_launch();
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over 64 channels, eps as an argument; the pixel-shuffle + base-image epilogue
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void esc_layernorm_kernel(const float* __restrict__ x, T* __restrict__ y, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int64_t npix, int ldx, int ldy) {
    constexpr int C = ECF_C;
    const int v = threadIdx.x & 15;
    const f32x4 gam = *reinterpret_cast<const f32x4*>(gamma + 4 * v), bet = *reinterpret_cast<const f32x4*>(beta + 4 * v);
    const int64_t trips = (npix + 15) / 16;   // 16 pixels per trip of a 256-thread group; every lane runs every trip of its group
    for (int64_t t = (int64_t)blockIdx.x; t < trips; t += gridDim.x) {
        const int64_t px = 16 * t + (threadIdx.x >> 4);
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (px < npix) r = *reinterpret_cast<const f32x4*>(x + px * ldx + 4 * v);
        const float mean = row_sum16((r[0] + r[1]) + (r[2] + r[3])) * (1.0f / C);
        const f32x4 c = r - mean;
        const float var = row_sum16((c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3])) * (1.0f / C);
        r = c * (1.0f / sqrtf(var + eps)) * gam + bet;
        if (px < npix) Vec4<T>::store(y + px * ldy + 4 * v, r);
    }
}

__global__ __launch_bounds__(256) void esc_shuffle_add_kernel(const float* __restrict__ rows, const float* __restrict__ x, float* __restrict__ y,
                                                              int H, int W, int s, int ld, int64_t total) {
    const int Hs = H * s, Ws = W * s;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % Ws), Y = (int)((i / Ws) % Hs), c = (int)((i / ((int64_t)Ws * Hs)) % 3);
        const int64_t b = i / ((int64_t)Ws * Hs * 3);
        const int yy = Y / s, xx = X / s;
        const int64_t px = (b * H + yy) * W + xx;
        y[i] = rows[px * ld + c * s * s + (Y % s) * s + X % s] + x[((b * 3 + c) * H + yy) * (int64_t)W + xx];
    }
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

extern "C" int hat_esc_convffn_tiles(int32_t H, int32_t W) {
    if (H < 1 || W < 1) return HAT_EINVAL;
    return ((H + ECF_TH - 1) / ECF_TH) * ((W + ECF_TW - 1) / ECF_TW);
}

extern "C" int hat_esc_convffn(const HatEscConvFfnDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatEscConvFfnDesc& d = *dp;
    if (d.dtype != HAT_F32 && d.dtype != HAT_BF16) return HAT_EINVAL;
    if (d.B < 1 || d.B > 65535 || d.H < 1 || d.W < 1 || d.reserved0) return HAT_EINVAL;
    if (d.hid_p != 96 && d.hid_p != 128) return HAT_EUNSUPPORTED;
    if (!d.x || !d.w1 || !d.b1 || !d.dww || !d.dwb || !d.w2 || !d.b2 || !d.out || d.out == d.x) return HAT_EINVAL;
    if (!aligned(d.x, 16) || !aligned(d.w1, 16) || !aligned(d.b1, 16) || !aligned(d.dww, 16) || !aligned(d.dwb, 16) || !aligned(d.w2, 16)
        || !aligned(d.b2, 16) || !aligned(d.out, 16)) return HAT_EINVAL;
    if (d.ldx < ECF_C || d.ldx % 4) return HAT_EINVAL;
    const int ovec = (d.dtype == HAT_BF16 && !d.out_f32) ? 8 : 4;
    if (d.ldo < ECF_C || d.ldo % ovec) return HAT_EINVAL;
    if ((d.ln_g == nullptr) != (d.ln_b == nullptr)) return HAT_EINVAL;
    if (d.ln_g && (!aligned(d.ln_g, 16) || !aligned(d.ln_b, 16) || !(d.ln_eps > 0.f))) return HAT_EINVAL;
    if (d.r && (!aligned(d.r, 16) || d.ldr < ECF_C || d.ldr % 4)) return HAT_EINVAL;
    if (d.partials && !aligned(d.partials, 16)) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.hid_p == 96 ? esc_convffn_launch<bf16_t, 96>(d, s) : esc_convffn_launch<bf16_t, 128>(d, s);
    return d.hid_p == 96 ? esc_convffn_launch<float, 96>(d, s) : esc_convffn_launch<float, 128>(d, s);
}

extern "C" int hat_window_attention_r(const void* q, const void* kv, const float* bias, void* out, int32_t B, int32_t h, int32_t w,
                                      int32_t C, int32_t heads, int32_t ws, int32_t ldq, int32_t ldkv, int32_t ldo, int32_t dtype,
                                      void* stream) {
    if (!q || !kv || !bias || !out || B < 1 || B > 65535 || h < 1 || w < 1) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (ws != WAR_WS || heads < 1 || C != heads * WAR_D) return HAT_EUNSUPPORTED;
    const int vec = dtype == HAT_BF16 ? 8 : 4;
    if (ldq < C || ldq % vec || ldkv < 2 * C || ldkv % vec || ldo < C || ldo % vec) return HAT_EINVAL;
    if (!aligned(q, 16) || !aligned(kv, 16) || !aligned(out, 16) || !aligned(bias, 4)) return HAT_EINVAL;
    const int Hp = (h + WAR_WS - 1) / WAR_WS * WAR_WS, Wp = (w + WAR_WS - 1) / WAR_WS * WAR_WS;
    if (Hp - h > h - 1 || Wp - w > w - 1) return HAT_EINVAL;   // a reflection reaches at most the first row / column
    WarArgs a{q, kv, bias, out, h, w, C, heads, Wp / WAR_WS, ldq, ldkv, ldo};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return dtype == HAT_BF16 ? window_attention_r_launch<bf16_t>(a, B, s) : window_attention_r_launch<float>(a, B, s);
}

extern "C" int hat_esc_layernorm(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx,
                                 int32_t ldy, int32_t dtype, void* stream) {
    if (!x || !y || !gamma || !beta || npix < 1 || !(eps > 0.f)) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (ldx < ECF_C || ldx % 4 || ldy < ECF_C || ldy % 4) return HAT_EINVAL;
    if (!aligned(x, 16) || !aligned(y, 8) || !aligned(gamma, 16) || !aligned(beta, 16)) return HAT_EINVAL;
    const int64_t trips = (npix + 15) / 16;
    const int grid = (int)(trips < 4096 ? trips : 4096);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == HAT_BF16)
        HAT_LAUNCH(esc_layernorm_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, x, reinterpret_cast<bf16_t*>(y), gamma, beta, eps, npix, ldx, ldy);
    else
        HAT_LAUNCH(esc_layernorm_kernel<float>, dim3(grid), dim3(256), 0, s, x, reinterpret_cast<float*>(y), gamma, beta, eps, npix, ldx, ldy);
    return hat_check_launch();
}

extern "C" int hat_esc_shuffle_add(const float* rows, const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t s, int32_t ld,
                                   void* stream) {
    if (!rows || !x || !y || B < 1 || H < 1 || W < 1 || s < 1 || s > 8 || ld < 3 * s * s) return HAT_EINVAL;
    const int64_t total = (int64_t)B * 3 * H * s * W * s;
    const int64_t blocks = (total + 255) / 256;
    HAT_LAUNCH(esc_shuffle_add_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
               rows, x, y, H, W, s, ld, total);
    return hat_check_launch();
}
