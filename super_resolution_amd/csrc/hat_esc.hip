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
// The ConvFFN and LayerNorm kernels are templates on the channel count in hat_esc_ffn.h (hat_escfp.hip instantiates them at 48);
// their 64-channel entry points are here.
// Contracts: include/hat_mi355x.h "ESC".  DESIGN.md 4.14.
#include "hat_esc_ffn.h"   // the ConvFFN and LayerNorm kernels, shared with hat_escfp.hip

namespace {

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
// The pixel-shuffle + base-image epilogue (the LayerNorm over 64 channels is hat_esc_ffn.h's)
// ---------------------------------------------------------------------------------------------
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

constexpr int ECF_C = 64;

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
    if (const int e = esc_convffn_check(d, ECF_C)) return e;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.hid_p == 96 ? esc_convffn_launch<bf16_t, ECF_C, 96>(d, s) : esc_convffn_launch<bf16_t, ECF_C, 128>(d, s);
    return d.hid_p == 96 ? esc_convffn_launch<float, ECF_C, 96>(d, s) : esc_convffn_launch<float, ECF_C, 128>(d, s);
}

extern "C" int hat_window_attention_r(const void* q, const void* kv, const float* bias, void* out, int32_t B, int32_t h, int32_t w,
                                      int32_t C, int32_t heads, int32_t ws, int32_t ldq, int32_t ldkv, int32_t ldo, int32_t dtype,
                                      void* stream) {
    if (!q || !kv || !bias || !out || B < 1 || B > 65535 || h < 1 || w < 1) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (ws != WAR_WS || heads < 1 || C != heads * WAR_D) return HAT_EUNSUPPORTED;
    const int vec = dtype == HAT_BF16 ? 8 : 4;
    if (ldq < C || ldq % vec || ldkv < 2 * C || ldkv % vec || ldo < C || ldo % vec) return HAT_EINVAL;
    if (!esc_aligned(q, 16) || !esc_aligned(kv, 16) || !esc_aligned(out, 16) || !esc_aligned(bias, 4)) return HAT_EINVAL;
    const int Hp = (h + WAR_WS - 1) / WAR_WS * WAR_WS, Wp = (w + WAR_WS - 1) / WAR_WS * WAR_WS;
    if (Hp - h > h - 1 || Wp - w > w - 1) return HAT_EINVAL;   // a reflection reaches at most the first row / column
    WarArgs a{q, kv, bias, out, h, w, C, heads, Wp / WAR_WS, ldq, ldkv, ldo};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return dtype == HAT_BF16 ? window_attention_r_launch<bf16_t>(a, B, s) : window_attention_r_launch<float>(a, B, s);
}

extern "C" int hat_esc_layernorm(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx,
                                 int32_t ldy, int32_t dtype, void* stream) {
    return esc_layernorm_run<ECF_C>(x, y, gamma, beta, eps, npix, ldx, ldy, dtype, stream);
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
