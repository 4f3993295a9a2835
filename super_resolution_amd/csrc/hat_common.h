// hat_common.h — device-side helpers shared by the gfx950 kernels (wave64, MFMA 16x16 tiles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hat_mi355x.h"

typedef __bf16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte piece

#define HAT_LDS_MAX 163840  // 160 KiB per workgroup on gfx950

// ---------------------------------------------------------------------------------------------
// MT<T>: one "k-step" of 32 along K on a 16x16 output tile.
//   bf16: one v_mfma_f32_16x16x32_bf16; lane l holds A[row l&15][k = 8*(l>>4)+j], j = 0..7
//   f32 : eight v_mfma_f32_16x16x4_f32; element j of every lane feeds MFMA j, which contracts
//         over k = 8*g + j, g = l>>4 = 0..3 — the same (g, j) -> k map as bf16, so LDS layouts
//         and fragment addressing are shared by both instantiations.  The f32 form is bit-wise
//         an fp32 fmaf chain (exact-fp32 parity path), 1/16 of the bf16 rate.
//   D layout (both): col = l & 15 (B's column), row = 4*(l>>4) + reg (A's row).
// ---------------------------------------------------------------------------------------------
template <typename T> struct MT;

template <> struct MT<bf16_t> {
    static constexpr int VEC = 8;   // elements per 16 bytes
    static constexpr int KC = 64;   // K elements per staged weight chunk (128 B per row)
    typedef bf16_t frag_t __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ frag_t load(const bf16_t* p) { return *reinterpret_cast<const frag_t*>(p); }
    static __device__ __forceinline__ frag_t zero() {
        frag_t z;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = (bf16_t)0.0f;
        return z;
    }
    static __device__ __forceinline__ f32x4 mma(frag_t a, frag_t b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    // half k-step (16 deep): v_mfma_f32_16x16x16_bf16, lane l holds A[row l&15][k = 4*(l>>4)+j], j = 0..3
    typedef short half_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ half_t load_half(const bf16_t* p) { return *reinterpret_cast<const half_t*>(p); }
    static __device__ __forceinline__ f32x4 mma_half(half_t a, half_t b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    }
};

template <> struct MT<float> {
    static constexpr int VEC = 4;
    static constexpr int KC = 32;
    typedef float frag_t __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ frag_t load(const float* p) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(p + 4);
        frag_t r;
        r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
        r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
        return r;
    }
    static __device__ __forceinline__ frag_t zero() {
        frag_t z;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = 0.0f;
        return z;
    }
    static __device__ __forceinline__ f32x4 mma(frag_t a, frag_t b, f32x4 c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
    // half k-step (16 deep): four 16x16x4 MFMAs, element j <-> k = 4*(l>>4)+j
    typedef f32x4 half_t;
    static __device__ __forceinline__ half_t load_half(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ f32x4 mma_half(half_t a, half_t b, f32x4 c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
};

// conversions ---------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T to_T(float v);
template <> __device__ __forceinline__ float to_T<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t to_T<bf16_t>(float v) { return (bf16_t)v; }  // RNE, v_cvt_pk_bf16_f32
__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(bf16_t v) { return (float)v; }

// 4 consecutive T values <-> 4 floats
template <typename T> struct Vec4;
template <> struct Vec4<float> {
    typedef f32x4 raw_t;  // load_raw / cvt split a load from its conversion, so a batch of loads can stay in flight
    static __device__ __forceinline__ raw_t load_raw(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ f32x4 cvt(raw_t r) { return r; }
    static __device__ __forceinline__ f32x4 load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void store(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
};
template <> struct Vec4<bf16_t> {
    typedef bf16_t v4 __attribute__((ext_vector_type(4)));
    typedef v4 raw_t;
    static __device__ __forceinline__ raw_t load_raw(const bf16_t* p) { return *reinterpret_cast<const v4*>(p); }
    static __device__ __forceinline__ f32x4 cvt(raw_t h) {
        f32x4 r;
        r[0] = (float)h[0]; r[1] = (float)h[1]; r[2] = (float)h[2]; r[3] = (float)h[3];
        return r;
    }
    static __device__ __forceinline__ f32x4 load(const bf16_t* p) {
        const v4 h = *reinterpret_cast<const v4*>(p);
        f32x4 r;
        r[0] = (float)h[0]; r[1] = (float)h[1]; r[2] = (float)h[2]; r[3] = (float)h[3];
        return r;
    }
    static __device__ __forceinline__ void store(bf16_t* p, f32x4 v) {
        v4 h;
        h[0] = (bf16_t)v[0]; h[1] = (bf16_t)v[1]; h[2] = (bf16_t)v[2]; h[3] = (bf16_t)v[3];
        *reinterpret_cast<v4*>(p) = h;
    }
};

// The value a stored T holds: what a pool over a stored map must add (the ESC pool, esc_arch.py:96,121, is a mean of the very
// tensor the 13x13 conv then reads — here the T-rounded LayerNorm output; pooling the unrounded fp32 values instead makes the
// pool depend on WHO computes it: a band-sharded frame pools the stored rows).
template <typename T> __device__ __forceinline__ f32x4 as_stored(f32x4 v) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)(bf16_t)v[r];
    }
    return v;
}

// Two adjacent n-tiles' accumulators of one pixel -> ONE 16-byte bf16 store per lane.  In the MFMA D layout lane group g
// holds channels 4g..4g+3 of every n-tile, so a plain store is 8 bytes per lane and 32 contiguous bytes per pixel.
// v_permlane16_swap exchanges the odd 16-lane rows of its first operand with the even rows of its second: afterwards an
// even lane group holds 8 consecutive channels of tile `nt`, an odd one 8 consecutive channels of tile `nt + 1`, and one
// store instruction writes 64 contiguous bytes per pixel.  All 64 lanes must be active.  `row` = the pixel's output row,
// n0 = first channel of tile nt; needs 16-byte aligned rows.
__device__ __forceinline__ void store_pair_bf16(bf16_t* row, int n0, int g, f32x4 a, f32x4 b) {
    typedef bf16_t v4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const v4 ha = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3]};
    const v4 hb = {(bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
    const u32x2 ua = __builtin_bit_cast(u32x2, ha), ub = __builtin_bit_cast(u32x2, hb);
    const auto r0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    const u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
    const int n = (g & 1) ? n0 + 16 + 4 * (g - 1) : n0 + 4 * g;
    *reinterpret_cast<u32x4*>(row + n) = v;
}
// the same with a per-lane store predicate (the lane exchange itself always runs on all 64 lanes)
__device__ __forceinline__ void store_pair_bf16_if(bf16_t* row, int n0, int g, f32x4 a, f32x4 b, bool pred) {
    typedef bf16_t v4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const v4 ha = {(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3]};
    const v4 hb = {(bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
    const u32x2 ua = __builtin_bit_cast(u32x2, ha), ub = __builtin_bit_cast(u32x2, hb);
    const auto r0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    const u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
    const int n = (g & 1) ? n0 + 16 + 4 * (g - 1) : n0 + 4 * g;
    if (pred) *reinterpret_cast<u32x4*>(row + n) = v;
}

// ... and for FP16 rows (the 16-bit residual stream, hat_hab_tail3): round to nearest even, clamped to the finite FP16 range
__device__ __forceinline__ void store_pair_f16_if(_Float16* row, int n0, int g, f32x4 a, f32x4 b, bool pred) {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    auto c = [](float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f); };
    const v4 ha = {c(a[0]), c(a[1]), c(a[2]), c(a[3])};
    const v4 hb = {c(b[0]), c(b[1]), c(b[2]), c(b[3])};
    const u32x2 ua = __builtin_bit_cast(u32x2, ha), ub = __builtin_bit_cast(u32x2, hb);
    const auto r0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    const u32x4 v = {r0[0], r1[0], r0[1], r1[1]};
    const int n = (g & 1) ? n0 + 16 + 4 * (g - 1) : n0 + 4 * g;
    if (pred) *reinterpret_cast<u32x4*>(row + n) = v;
}

// Four channels of an FP16 row as raw bits (8 bytes).  Loads of the FP16 residual stream keep their results in an INTEGER
// array until use: parked in float registers through a bit_cast, hipcc once merged the two dwords.
typedef unsigned h4raw __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h4raw load_h4raw(const void* p) { return *reinterpret_cast<const h4raw*>(p); }
__device__ __forceinline__ float h16bits_to_f(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
// exact.  Scalar shifts, no <2 x half> view of the dwords: through such a view hipcc (in the group conv's epilogue) again
// converted the first dword twice and never read the second.
__device__ __forceinline__ f32x4 h4raw_to_f32(h4raw r) {
    const unsigned a = r[0], b = r[1];
    return f32x4{h16bits_to_f(a & 0xffffu), h16bits_to_f(a >> 16), h16bits_to_f(b & 0xffffu), h16bits_to_f(b >> 16)};
}
// four channels -> FP16 (round to nearest even, clamped to the finite range), one 8-byte store
__device__ __forceinline__ void store_h4(_Float16* p, f32x4 v) {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    auto c = [](float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f); };
    *reinterpret_cast<v4*>(p) = v4{c(v[0]), c(v[1]), c(v[2]), c(v[3])};
}

// ---- the FP16-range guard of the residual stream (hat_hab_tail3_guarded, hat_conv_guarded, hat_linear_guarded) ----
// The guarded form of a kernel that stores FP16 rows takes one more argument, `unsigned* sat`, as a template parameter pack
// beside TH: the pack is empty in the unguarded instantiations, whose signature, arguments and code are what they were.
template <typename... S> __device__ __forceinline__ unsigned* sat_arg(S... s) {
    static_assert(sizeof...(S) <= 1, "at most one guard slot");
    if constexpr (sizeof...(S) == 1) return (s, ...);
    else return nullptr;
}
// Running maximum of |v| over the fp32 values a lane is about to convert: two v_maximum3_f32 with abs modifiers per four
// values.  The IEEE-754-2019 maximum, not fmax: a NaN stays a NaN.
__device__ __forceinline__ float sat_max4(float m, f32x4 v) {
    m = __builtin_elementwise_maximum(__builtin_elementwise_maximum(m, __builtin_fabsf(v[0])), __builtin_fabsf(v[1]));
    return __builtin_elementwise_maximum(__builtin_elementwise_maximum(m, __builtin_fabsf(v[2])), __builtin_fabsf(v[3]));
}
// After the stores: m = the lane's maximum (>= 0, or a NaN).  !(m <= 65504) holds for a larger magnitude, an infinity and a
// NaN.  In range — no lane of the wave trips — this is one compare and one branch.  Otherwise the wave reduces the bit patterns
// (as unsigned they order like the magnitudes, a NaN above the infinity) and ONE lane raises *sat to the largest with a global
// atomic; *sat keeps the largest over all waves and launches since it was last zeroed.  All 64 lanes must be active.
__device__ __forceinline__ void sat_report(unsigned* sat, float m, int lane) {
    if (__builtin_amdgcn_ballot_w64(!(m <= 65504.0f)) != 0) {
        unsigned u = __float_as_uint(m) & 0x7fffffffu;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, off));
        if (lane == 0) atomicMax(sat, u);
    }
}

// LDS row stride (in elements) for rows of `n` elements of size `es`, for MFMA operand images read by ds_read_b128
// with lane (c16, g) -> row base + c16, 16-byte slot k0 + g (bf16) or k0 + 2g (+1) (f32).  The instruction is serviced
// in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,...}: rows 0-3 and 12-15 of lane group g together
// with rows 4-11 of lane group g^1.  Enumerating all base alignments (tools: DESIGN.md 4.1): with 2-byte elements a
// stride of S slots is conflict-free exactly when S % 4 == 2 (odd strides, the textbook padding, are 2-way on every
// read); with 4-byte elements nothing beats an odd stride (2-way).
__host__ __device__ constexpr int lds_row_elems(int n, int es) {
    int slots = (n * es + 15) / 16;
    if (es == 2) slots += (6 - slots % 4) % 4;    // -> slots % 4 == 2
    else if ((slots & 1) == 0) slots += 1;
    return slots * 16 / es;
}

// Sum over the 16 lanes of a DPP row (lanes 16r .. 16r+15), result in every lane: four v_add_f32 with row_ror
// modifiers instead of four ds_bpermute round trips (__shfl_xor).  Deterministic; order differs from a butterfly.
__device__ __forceinline__ float row_sum16(float s) {
    s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x128, 0xf, 0xf, false));
    s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x124, 0xf, 0xf, false));
    s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x122, 0xf, 0xf, false));
    s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x121, 0xf, 0xf, false));
    return s;
}

// Workgroup barrier for LDS hand-offs that leaves global loads in flight.  __syncthreads() also drains vmcnt, which
// turns every prefetch issued before it into a full memory round trip at the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// erf-GELU for T-typed (bf16) outputs: erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below a bf16 ulp) with
// raw v_exp/v_rcp: ~16 VALU instructions instead of libdevice erff's ~50, which made the 288-wide GELU linear VALU-bound.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);
    const float erf_abs = fmaf(-p * t, e, 1.0f);          // erf(|x| / sqrt 2)
    return 0.5f * x + 0.5f * fabsf(x) * erf_abs;           // 0.5 x (1 + sign(x) erf_abs)
}
template <typename T> __device__ __forceinline__ float gelu_act(float x) {
    if constexpr (sizeof(T) == 2) return gelu_erf_fast(x);
    else return gelu_erf(x);
}

// Launch status.  Every launch site first drains hipGetLastError(): the value is per-thread state that
// other libraries in the process (e.g. a failed probe inside the framework) may have left set.
// tensor2img of the reference (basicsr utils/img_util.py:66-91): clamp to [0, 1], x255 in fp32, round half to even
// (v_rndne_f32).  The one conversion every 8-bit output path shares (hat_planes_to_u8, hat_conv3x3_to_u8).
__device__ __forceinline__ unsigned hat_unit_to_u8(float v) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (unsigned)(int)__builtin_rintf(v * 255.0f);
}

// float(v) / 255.0f for every byte value, correctly rounded: built by the compiler's constant evaluator (IEEE), so a
// kernel does not depend on how the device divides (a reciprocal multiply is not exact for every byte value).  The 8-bit
// input side (hat_u8_to_planes) and the Y value of the metrics (hat_u8_metrics) read the same table.
struct HatU8Table {
    float v[256];
    constexpr HatU8Table() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
    }
};
static __device__ const HatU8Table hat_u8_unit{};

// 4:2:0 YCbCr <-> RGB (definition: super_resolution_amd/yuv.py).  A 3 x 4 matrix travels by value in the kernel arguments.
// Every product and sum is rounded to fp32 on its own — contraction is off inside these functions — so that numpy float32
// arithmetic reproduces them bit for bit; every route (hat_yuv.hip's kernels, conv_last's yuv epilogues) calls these.
struct HatCsc { float m[12]; };

// Y, Cb - 128, Cr - 128 in byte units (any sample width: an n-bit code times 2^(8 - n)) -> r, g, b in [0, 1]: rows R, G, B;
// columns Y, Cb', Cr', offset (added last).  The one expression of the byte and the deep path.
__device__ __forceinline__ void hat_ycc_to_rgb_f(const HatCsc& k, float y, float cb, float cr, float (&rgb)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = ((k.m[4 * c] * y + k.m[4 * c + 1] * cb) + k.m[4 * c + 2] * cr) + k.m[4 * c + 3];
        rgb[c] = fminf(fmaxf(v, 0.f), 1.f);
    }
}

// bytes Y, Cb, Cr -> r, g, b in [0, 1]
__device__ __forceinline__ void hat_ycc_to_rgb(const HatCsc& k, unsigned Y, unsigned Cb, unsigned Cr, float (&rgb)[3]) {
#pragma clang fp contract(off)
    const float y = (float)Y, cb = (float)Cb - 128.0f, cr = (float)Cr - 128.0f;
    hat_ycc_to_rgb_f(k, y, cb, cr, rgb);
}

// n-bit codes Y, Cb, Cr -> r, g, b in [0, 1]; inv = 2^(8 - n): the products with it and the centring are exact
__device__ __forceinline__ void hat_ycc_to_rgb(const HatCsc& k, unsigned Y, unsigned Cb, unsigned Cr, float inv, float (&rgb)[3]) {
#pragma clang fp contract(off)
    const float y = (float)Y * inv, sb = (float)Cb * inv, sr = (float)Cr * inv;
    const float cb = sb - 128.0f, cr = sr - 128.0f;
    hat_ycc_to_rgb_f(k, y, cb, cr, rgb);
}

// the float path's r, g, b of one pixel -> Y (with its offset) and the pixel's cb, cr terms (without: the offset joins
// after the 2 x 2 average); rows Y, Cb, Cr; columns R, G, B, offset
__device__ __forceinline__ void hat_rgb_to_ycc(const HatCsc& k, float r, float g, float b, float& Y, float& cb, float& cr) {
#pragma clang fp contract(off)
    r = fminf(fmaxf(r, 0.f), 1.f);
    g = fminf(fmaxf(g, 0.f), 1.f);
    b = fminf(fmaxf(b, 0.f), 1.f);
    Y = ((k.m[0] * r + k.m[1] * g) + k.m[2] * b) + k.m[3];
    cb = (k.m[4] * r + k.m[5] * g) + k.m[6] * b;
    cr = (k.m[8] * r + k.m[9] * g) + k.m[10] * b;
}

// a value in byte units -> the byte: clamp to [0, 255], round half to even
__device__ __forceinline__ unsigned hat_ycc_byte(float v) { return (unsigned)(int)__builtin_rintf(fminf(fmaxf(v, 0.f), 255.f)); }

// a value in byte units -> the n-bit code: scale = 2^(n - 8) (the product is exact), clamp to [0, maxcode = 2^n - 1], round
// half to even.  scale = 1, maxcode = 255 is hat_ycc_byte.
__device__ __forceinline__ unsigned hat_ycc_code(float v, float scale, float maxcode) {
#pragma clang fp contract(off)
    const float s = v * scale;
    return (unsigned)(int)__builtin_rintf(fminf(fmaxf(s, 0.f), maxcode));
}

// the chroma value (byte units) of a 2 x 2 block from its two row sums (left + right each): (top + bottom) * 0.25 + offset
__device__ __forceinline__ float hat_chroma_value(float top, float bottom, float offset) {
#pragma clang fp contract(off)
    const float s = top + bottom;
    const float q = s * 0.25f;
    return q + offset;
}
__device__ __forceinline__ unsigned hat_chroma_byte(float top, float bottom, float offset) { return hat_ycc_byte(hat_chroma_value(top, bottom, offset)); }

// the chroma value of a 4:2:2 pair from its sum (left + right): sum * 0.5 + offset; a 4:4:4 sample is hat_add_rn(c, offset)
__device__ __forceinline__ float hat_chroma_value_h(float sum, float offset) {
#pragma clang fp contract(off)
    const float q = sum * 0.5f;
    return q + offset;
}

__device__ __forceinline__ float hat_add_rn(float a, float b) {   // a sum that stays a sum whatever surrounds the call
#pragma clang fp contract(off)
    return a + b;
}

// Chroma siting (yuv.py, "Chroma siting").  In: the chroma of one source pixel from the (up to) four samples around it, in byte
// units, centred on 128: every step is exact.  Out: the [1 2 1] tap of a co-sited axis from (left, centre, right) or (above,
// row, below), and value = tap sum * scale + offset with scale a power of two.
__device__ __forceinline__ float hat_chroma_up4(float s00, float s01, float s10, float s11) {
#pragma clang fp contract(off)
    const float top = s00 + s01, bottom = s10 + s11;
    const float q = (top + bottom) * 0.25f;
    return q - 128.0f;
}
__device__ __forceinline__ float hat_chroma_tap121(float before, float centre, float after) {
#pragma clang fp contract(off)
    const float outer = before + after;
    const float mid = 2.0f * centre;
    return outer + mid;
}
__device__ __forceinline__ float hat_chroma_value_s(float sum, float scale, float offset) {
#pragma clang fp contract(off)
    const float q = sum * scale;
    return q + offset;
}

#define HAT_LAUNCH(...)                      \
    do {                                     \
        (void)hipGetLastError();             \
        hipLaunchKernelGGL(__VA_ARGS__);     \
    } while (0)

static inline int hat_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
