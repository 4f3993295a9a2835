// hat_gated_ffn.h — what the three HAB tail kernels share of the gated depthwise FFN: hat_ffn2.hip (second generation,
// embed_dim 144), hat_tail3.hip (third generation, 144) and hat_tail3l.hip (third generation, 180).  The fp16 / LDS helpers,
// the start of the depthwise accumulators, the SiLU gate feeding the fp16 fc2 MFMAs, and the host-side argument check and
// launch.  Stage 0, fc1, the depthwise walk, the epilogue and the GAP reduction stay with each kernel: DESIGN.md 4.0d says why.
//
// Lane roles, as in the kernels: lane = (c16, g) = (lane & 15, lane >> 4); a wave owns tile rows 2 wave, 2 wave + 1.
#pragma once
#include "hat_common.h"

namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) char lds_char;

__device__ __forceinline__ u32x4 lds_rd16(unsigned addr) { return *(__attribute__((address_space(3))) const u32x4*)(uintptr_t)addr; }
__device__ __forceinline__ h2 as_h2(unsigned v) { return __builtin_bit_cast(h2, v); }
__device__ __forceinline__ unsigned as_u(h2 v) { return __builtin_bit_cast(unsigned, v); }
// one LDS-DMA piece: 64 lanes x 16 B from src (wave-uniform) + lane_off -> 1 KiB at dst (wave-uniform)
__device__ __forceinline__ void dma1k(const char* src, unsigned lane_off, char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + lane_off),
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
// 16 readable zero bytes: where stage 0's im2col of c1 points a tap that lies outside the image
__device__ __attribute__((aligned(16))) unsigned hat_gffn_zero_page[4] = {0, 0, 0, 0};

// Depthwise accumulators of the wave's two tile rows, [tile row][dword]: a-units / gate-units 8g..8g+7, two per dword.  They
// start as the depthwise bias: "tap 9" of the lane group's record [tap 0..8, bias][a-units 8 | gate-units 8] fp16 at wdad.
__device__ __forceinline__ void dw_init(unsigned wdad, h2 (&da)[2][4], h2 (&dg)[2][4]) {
    const u32x4 ba = lds_rd16(wdad + 9 * 32), bg = lds_rd16(wdad + 9 * 32 + 16);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int k = 0; k < 4; ++k) { da[pt][k] = as_h2(ba[k]); dg[pt][k] = as_h2(bg[k]); }
}

// a * SiLU(g) of one tile row in packed fp16 (v_exp_f16 / v_rcp_f16): the result IS the fc2 MFMA's B fragment, natural k order
__device__ __forceinline__ h8 gate_silu(const h2 (&a)[4], const h2 (&gt)[4]) {
    u32x4 gu;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const h2 x = gt[k];
        const h2 tt = x * (h2){(_Float16)-1.4426950408889634f, (_Float16)-1.4426950408889634f};
        h2 e = {(_Float16)__builtin_exp2f16(tt[0]), (_Float16)__builtin_exp2f16(tt[1])};
        e = e + (h2){(_Float16)1.0f, (_Float16)1.0f};
        const h2 r = {(_Float16)__builtin_amdgcn_rcph(e[0]), (_Float16)__builtin_amdgcn_rcph(e[1])};
        gu[k] = as_u(a[k] * (x * r));                  // a * g * sigmoid(g)
    }
    return __builtin_bit_cast(h8, gu);
}

// Phase C of the third generation: the chunk's fc2 fragments [NT][1 KiB] from LDS at w2ad (requested first, consumed after
// the gate math), the gate, NT x 2 fp16 MFMAs into the persistent accumulators.
template <int NT>
__device__ __forceinline__ void gate_fc2(unsigned w2ad, const h2 (&da)[2][4], const h2 (&dg)[2][4], f32x4 (&acc2)[NT][2]) {
    h8 a2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) a2[nt] = __builtin_bit_cast(h8, lds_rd16(w2ad + (unsigned)(nt * 1024)));
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const h8 gf = gate_silu(da[pt], dg[pt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc2[nt][pt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[nt], gf, acc2[nt][pt], 0, 0, 0);
    }
}

// ---- host side ----
// the epilogue's optional outputs: with ln1_g set, ln1_b / n_out / ldn / gap_c must describe them
inline bool hat_ln1_args_ok(const HatFfnDesc& d) {
    return !d.ln1_g || (d.ln1_b && d.n_out && d.ldn >= d.C && d.ldn % 4 == 0 && d.gap_c >= 0 && d.gap_c <= 16 && d.gap_c % 4 == 0);
}
// one 256-thread workgroup per 16 x `rows` pixel tile and sample, `lds` bytes of dynamic LDS
// (more...: the guarded form's slot, hat_tail3.hip)
template <typename Aggr, typename... More>
int hat_tail_launch(void (*kern)(const HatFfnDesc, const Aggr, More...), int lds, int rows, const HatFfnDesc& d, const Aggr& ag, void* stream,
                    More... more) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    dim3 grid((d.W + 15) / 16, (d.H + rows - 1) / rows, d.B);
    HAT_LAUNCH(kern, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(stream), d, ag, more...);
    return hat_check_launch();
}

}  // namespace
