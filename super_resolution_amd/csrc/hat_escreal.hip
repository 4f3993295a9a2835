// hat_escreal.hip — what ESCReal (esc_real_arch.py:402-475) adds to ESC's kernels, on gfx950.
//
//   hat_escreal_skip   out = [r +] skip(x), skip = 1x1 3->128, depthwise 7x7 with REFLECT padding, LeakyReLU(0.2), 1x1 128->64
//                      (esc_real_arch.py:460-465), fp32 rows out.  Two facts make it one small kernel:
//                      (1) a 1x1 conv commutes with reflect padding: the hidden map at a pad position IS the hidden map at the
//                          mirrored pixel, so the kernel gathers x at (reflect(y), reflect(x)) and no padded copy exists;
//                      (2) with reflect padding all 49 taps of every pixel are inside, so depthwise(1x1(x)) is ONE dense 7x7
//                          conv 3->128: weights dw[c][tap] * W0[c][ci] (K = 49 * 3 = 147) and the constant bias
//                          b0[c] * sum_tap dw[c][tap] + bdw[c] (packing.escreal_skip_fold, fp32, host).
//                      Per 64-pixel tile: the (64, 147 -> 160) patch matrix in LDS, GEMM 160 -> 128 on the MFMA units, LeakyReLU,
//                      the (64, 128) hidden rows in LDS, GEMM 128 -> 64, + b3 [+ r].  Nothing 128 wide reaches HBM.
//   hat_dysample       the DySample head (esc_real_arch.py:361-399) after its three pointwise layers.  grid_sample(bilinear) and
//                      end_conv (1x1) are both linear, so end_conv runs first, per group, at LR size: rows hold, per LR pixel,
//                      [offset 8 s^2 | scope 8 s^2 | 4 groups x 3 projected values]; the 64-channel map at output size is never
//                      made.  Channel order of offset / scope / init_pos (the reference's view(B, 2, -1, H, W) followed by
//                      pixel_shuffle(s) and view(B, 2, 4, sH, sW)): entry d * 4 s^2 + grp * s^2 + i * s + j is axis d (0: x, 1: y)
//                      of group grp at output pixel (s y + i, s x + j).  Offsets are unbounded: the four corners are read from
//                      HBM wherever the clamped position lies, no tile or halo is assumed.
// Contracts: include/hat_mi355x.h "ESCReal".  DESIGN.md 4.15.
#include "hat_common.h"

namespace {

constexpr int ERS_C = 64, ERS_HID = 128, ERS_K = 147, ERS_KP = 160, ERS_PX = 64, ERS_THREADS = 256;

template <typename T> struct ErsLds {
    static constexpr int LDP = lds_row_elems(ERS_KP, sizeof(T));    // patch rows, MFMA operand
    static constexpr int LDH = lds_row_elems(ERS_HID, sizeof(T));   // hidden rows, MFMA operand
    static constexpr size_t PS = (size_t)ERS_PX * LDP * sizeof(T);
    static constexpr size_t BYTES = PS + (size_t)ERS_PX * LDH * sizeof(T);
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

struct ErsArgs {
    const float* x; const void* w1; const float* b1; const void* w3; const float* b3; const float* r; float* out;
    int H, W, ldr, ldo;
};

// LDS: [ ps: the 7x7x3 patches of 64 pixels as T [64][LDP] (k = 3 tap + ci, k >= 147 zero) | hs: lrelu(hidden) as T [64][LDH] ]
template <typename T>
__global__ __launch_bounds__(ERS_THREADS) void escreal_skip_kernel(const ErsArgs a) {
    typedef ErsLds<T> L;
    typedef typename MT<T>::frag_t frag_t;
    constexpr int KS1 = ERS_KP / 32, KS2 = ERS_HID / 32, LDP = L::LDP, LDH = L::LDH, PT = ERS_PX / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char ers_smem[];
    T* ps = reinterpret_cast<T*>(ers_smem);
    T* hs = reinterpret_cast<T*>(ers_smem + L::PS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int H = a.H, W = a.W, b = blockIdx.y;
    const int64_t n = (int64_t)H * W, p0 = (int64_t)blockIdx.x * ERS_PX;
    const float* xb = a.x + (int64_t)b * 3 * n;

    // ---- patches: position (y + ky - 3, x + kx - 3) past an edge reads the pixel it mirrors (H, W >= 4: one reflection suffices)
    for (int i = tid; i < ERS_PX * ERS_KP; i += ERS_THREADS) {
        const int p = i / ERS_KP, k = i % ERS_KP;
        float v = 0.f;
        if (k < ERS_K) {
            const int64_t px = min(p0 + p, n - 1);   // (the pixels of the last tile past the frame are computed and dropped)
            const int tap = k / 3, ci = k % 3;
            int yy = (int)(px / W) + tap / 7 - 3, xx = (int)(px % W) + tap % 7 - 3;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
            xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
            v = xb[(int64_t)ci * n + (int64_t)yy * W + xx];
        }
        ps[p * LDP + k] = to_T<T>(v);
    }
    __syncthreads();

    // ---- hidden = lrelu_0.2(Wf . patch + bf); wave w owns hidden channels 32 w .. 32 w + 31
    {
        const T* w1 = reinterpret_cast<const T*>(a.w1);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int ot = 2 * wave + o;
            frag_t af[KS1];
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) af[ks] = MT<T>::load(w1 + ((ot * KS1 + ks) * 64 + lane) * 8);
            const int ch = 16 * ot + 4 * g;
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(a.b1 + ch);
            for (int pt = 0; pt < PT; ++pt) {
                const int p = 16 * pt + l15;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) acc = MT<T>::mma(af[ks], MT<T>::load(ps + p * LDP + 32 * ks + 8 * g), acc);
                acc += b1;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = acc[r] >= 0.f ? acc[r] : 0.2f * acc[r];
                Vec4<T>::store(hs + p * LDH + ch, acc);
            }
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
            if (p0 + p < n) {
                const int64_t px = (int64_t)b * n + p0 + p;
                f32x4 v = acc + b3;
                if (a.r) v += *reinterpret_cast<const f32x4*>(a.r + px * a.ldr + ch);
                *reinterpret_cast<f32x4*>(a.out + px * a.ldo + ch) = v;
            }
        }
    }
}

template <typename T>
int escreal_skip_launch(const ErsArgs& a, int B, hipStream_t s) {
    constexpr size_t lds = ErsLds<T>::BYTES;
    auto kern = escreal_skip_kernel<T>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int64_t tiles = ((int64_t)a.H * a.W + ERS_PX - 1) / ERS_PX;
    HAT_LAUNCH(kern, dim3((unsigned)tiles, B), dim3(ERS_THREADS), lds, s, a);
    return hat_check_launch();
}

// ---------------------------------------------------------------------------------------------
// DySample: offsets -> sampling positions -> bilinear gather of the projected values
// ---------------------------------------------------------------------------------------------
struct DysArgs {
    const float* rows; const float* init_pos; const float* bias; float* y;
    int H, W, s, ld;
    int64_t total;   // B * sH * sW
};

// One axis of grid_sample(align_corners=False, padding_mode='border') for the reference's grid value of (c + 0.5 + off):
// normalise by the size, un-normalise, clamp to [0, size - 1] -> the lower corner, the upper one (clamped) and its weight.
// Every step is rounded on its own, as the reference's tensor ops are.
__device__ __forceinline__ void dys_axis(int c, float off, int size, int& i0, int& i1, float& t) {
#pragma clang fp contract(off)
    const float sz = (float)size;
    const float gn = 2.0f * (((float)c + 0.5f) + off) / sz - 1.0f;
    float p = (gn + 1.0f) * (sz * 0.5f) - 0.5f;
    p = fminf(fmaxf(p, 0.0f), sz - 1.0f);   // (fmaxf drops a NaN: the index below is always inside)
    const float f = floorf(p);
    i0 = (int)f;
    i1 = min(i0 + 1, size - 1);
    t = p - f;
}

__global__ __launch_bounds__(256) void dysample_kernel(const DysArgs a) {
    const int s = a.s, ss = s * s, H = a.H, W = a.W, Hs = H * s, Ws = W * s;
    const int o_scope = 8 * ss, o_proj = 16 * ss;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % Ws), Y = (int)((i / Ws) % Hs);
        const int64_t b = i / ((int64_t)Ws * Hs);
        const int yy = Y / s, xx = X / s, ij = (Y % s) * s + X % s;
        const float* base = a.rows + b * H * W * (int64_t)a.ld;
        const float* row = base + ((int64_t)yy * W + xx) * a.ld;
        float acc[3] = {a.bias[0], a.bias[1], a.bias[2]};
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const int mx = grp * ss + ij, my = 4 * ss + mx;
            float off[2];
            {
#pragma clang fp contract(off)
                off[0] = row[mx] * (1.0f / (1.0f + expf(-row[o_scope + mx]))) * 0.5f + a.init_pos[mx];
                off[1] = row[my] * (1.0f / (1.0f + expf(-row[o_scope + my]))) * 0.5f + a.init_pos[my];
            }
            int x0, x1, y0, y1;
            float tx, ty;
            dys_axis(xx, off[0], W, x0, x1, tx);
            dys_axis(yy, off[1], H, y0, y1, ty);
            const float* c00 = base + ((int64_t)y0 * W + x0) * a.ld + o_proj + 3 * grp;
            const float* c01 = base + ((int64_t)y0 * W + x1) * a.ld + o_proj + 3 * grp;
            const float* c10 = base + ((int64_t)y1 * W + x0) * a.ld + o_proj + 3 * grp;
            const float* c11 = base + ((int64_t)y1 * W + x1) * a.ld + o_proj + 3 * grp;
            const float w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty), w10 = (1.0f - tx) * ty, w11 = tx * ty;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (c00[c] * w00 + c01[c] * w01) + (c10[c] * w10 + c11[c] * w11);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.y[((b * 3 + c) * Hs + Y) * (int64_t)Ws + X] = acc[c];
    }
}

bool aligned(const void* p, uintptr_t al) { return reinterpret_cast<uintptr_t>(p) % al == 0; }

}  // namespace

extern "C" int hat_escreal_skip(const float* x, const void* w1, const float* b1, const void* w3, const float* b3, const float* r,
                                float* out, int32_t B, int32_t H, int32_t W, int32_t ldr, int32_t ldo, int32_t dtype, void* stream) {
    if (!x || !w1 || !b1 || !w3 || !b3 || !out) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (B < 1 || B > 65535 || H < 4 || W < 4) return HAT_EINVAL;   // reflect pad 3 needs a side of at least 4
    if (((int64_t)H * W + ERS_PX - 1) / ERS_PX > 0x7fffffff) return HAT_EINVAL;
    if (!aligned(x, 4) || !aligned(w1, 16) || !aligned(b1, 16) || !aligned(w3, 16) || !aligned(b3, 16) || !aligned(out, 16)) return HAT_EINVAL;
    if (ldo < ERS_C || ldo % 4) return HAT_EINVAL;
    if (r && (!aligned(r, 16) || ldr < ERS_C || ldr % 4)) return HAT_EINVAL;
    if (reinterpret_cast<const void*>(out) == reinterpret_cast<const void*>(x)) return HAT_EINVAL;
    const ErsArgs a{x, w1, b1, w3, b3, r, out, H, W, ldr, ldo};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return dtype == HAT_BF16 ? escreal_skip_launch<bf16_t>(a, B, s) : escreal_skip_launch<float>(a, B, s);
}

extern "C" int hat_dysample(const float* rows, const float* init_pos, const float* bias, float* y, int32_t B, int32_t H, int32_t W,
                            int32_t s, int32_t ld, void* stream) {
    if (!rows || !init_pos || !bias || !y || B < 1 || H < 1 || W < 1) return HAT_EINVAL;
    if (s < 2 || s > 4) return HAT_EUNSUPPORTED;
    if (ld < 16 * s * s + 12) return HAT_EINVAL;
    if (!aligned(rows, 4) || !aligned(init_pos, 4) || !aligned(bias, 4) || !aligned(y, 4)) return HAT_EINVAL;
    if ((int64_t)H * s > 0x7fffffff / ((int64_t)W * s)) return HAT_EINVAL;   // a plane's pixel count fits an int
    const int64_t total = (int64_t)B * H * s * W * s;
    const int64_t blocks = (total + 255) / 256;
    const DysArgs a{rows, init_pos, bias, y, H, W, s, ld, total};
    // tests/test_gpu_escreal_edges.py: DYS_TRIP_PIXELS = 16384 * 256 output pixels per trip
    HAT_LAUNCH(dysample_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return hat_check_launch();
}
