// hat_upfold.hip — the end of the network as ONE conv: the last Upsample conv (3x3, 64 -> 256), its PixelShuffle(2) and conv_last
// (3x3, 64 -> 3) are one linear map from the 64-channel map x at the shuffle's input size to the 2 x 2 x 3 output values of each of
// its pixels, with a 5 x 5 footprint (hat_arch.py:598-605, :856-858; contract: hat_upfold_to_* in include/hat_mi355x.h; the algebra
// and the border rule: packing.upfold_pieces / upfold_variant).  The 64-channel map at output size, which hat_conv wrote
// and conv_last's row sweep read back, does not exist.
//   * a persistent workgroup keeps the 50 A fragments (25 taps x 2 k-steps, 16 rows: 4 sub-pixels x (R, G, B, zero)) of the
//     interior weights in LDS, copied in once, and beside them the haloed input tile (20 x 36 pixels x 64 channels, the 16-byte
//     slots of a pixel swizzled by its column so that a row of 16 pixels reads conflict-free): no barrier inside the K loop;
//   * a wave owns 4 output rows x 16 columns and sweeps the tap rows for a fixed tap column: 8 input-row fragments and 5 weight
//     fragments feed 20 MFMAs;
//   * the next tile's input is fetched into registers before the K loop and written to LDS after it;
//   * pixels of the first / last row and column use other weights (a shift of the shuffled map that falls outside the image is
//     absent as a whole): after the main pass, border tiles recompute those pixels — one 16-pixel group per edge and column half,
//     under workgroup-uniform conditions — with the variant's fragments read from global memory, and the main pass does not store them;
//   * lane group g of an MFMA result holds R, G, B of output pixel 2 p + (g >> 1, g & 1): the planes store and the frame sink
//     (hat_frame_sink.h) take the same fp32 value (acc + bias) * out_scale + mean.
#include <type_traits>

#include "hat_frame_sink.h"

namespace {

constexpr int F_TR = 16, F_TC = 32, F_HALO = 2;
constexpr int F_HR = F_TR + 2 * F_HALO, F_HC = F_TC + 2 * F_HALO;       // 20 x 36 haloed pixels, 128 bytes each
constexpr int F_NFRAG = 50, F_WAVES = 8, F_THREADS = F_WAVES * 64;
constexpr int F_X_OFF = F_NFRAG * 1024;                                   // 51200
constexpr int F_LDS = F_X_OFF + F_HR * F_HC * 128;                        // 143360 bytes (one workgroup per CU)
constexpr int F_VARIANT = F_NFRAG * 512;                                  // bf16 elements of one variant's fragments
static_assert(F_LDS <= HAT_LDS_MAX, "weights + haloed tile must fit the LDS");

struct FoldEpi { float out_scale; float mean[3]; };
struct FoldEpiU8 { float out_scale; float mean[3]; int h_out, w_out, bgr; long long pitch, bstride; };
template <typename T, int SX, int SY, bool GREY> struct FoldEpiYuv {
    float out_scale; float mean[3]; int h_out, w_out; HatCsc k; HatSample<T> q; HatYuvDst<T> d;
};
template <typename E> struct FoldYuvTraits { static constexpr bool yuv = false, grey = false; static constexpr int sx = 1, sy = 1; };
template <typename T, int SX, int SY, bool G> struct FoldYuvTraits<FoldEpiYuv<T, SX, SY, G>> {
    static constexpr bool yuv = true, grey = G; static constexpr int sx = SX, sy = SY;
};

// byte offset of 16-byte slot s of haloed pixel (hy, hx) in the input tile
__device__ __forceinline__ unsigned fold_x_addr(int hy, int hx, int s) {
    return (unsigned)((hy * F_HC + hx) * 128 + ((s ^ ((hx >> 1) & 7)) << 4));
}

template <typename Epi>
__global__ __launch_bounds__(F_THREADS) void upfold_kernel(const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ wpk,
                                                           const float* __restrict__ bias, void* __restrict__ outv, int H, int W,
                                                           int tiles_x, int ntiles, Epi epi) {
    typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
    constexpr bool U8 = std::is_same<Epi, FoldEpiU8>::value;
    using YT = FoldYuvTraits<Epi>;
    constexpr bool YUV = YT::yuv;
    constexpr bool C420 = YUV && !YT::grey && YT::sx == 1 && YT::sy == 1, C422 = YUV && !YT::grey && YT::sx == 1 && YT::sy == 0;
    constexpr bool C444 = YUV && !YT::grey && YT::sx == 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const bf16_t* xb = x + (size_t)b * H * W * ldx;
    const int Ho = 2 * H, Wo = 2 * W;

    // ---- interior weights -> LDS, once (the first tile's barrier publishes them) ---------------------------------------------
    for (int i = tid; i < F_NFRAG * 64; i += F_THREADS)
        *reinterpret_cast<u32x4*>(smem + i * 16) = *reinterpret_cast<const u32x4*>(wpk + (size_t)i * 8);
    const f32x4 bias0 = *reinterpret_cast<const f32x4*>(bias + 4 * g);

    // ---- the epilogue of one 16-pixel group: this lane holds R, G, B of output pixel (2 py + (g >> 1), 2 px + (g & 1)) --------
    // Every lane of the wave calls it (the 4:2:0 / 4:2:2 chroma sums cross lane groups); `ok` says whether this lane's pixel is stored.
    auto finish = [&](f32x4 acc, f32x4 bs, int py, int px, bool ok) {
        const int oy = 2 * py + (g >> 1), ox = 2 * px + (g & 1);
        float rgb[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) rgb[m] = __builtin_fmaf(acc[m] + bs[m], epi.out_scale, epi.mean[m]);
        if constexpr (YUV) {
            float Yv, cbv, crv;
            hat_rgb_to_ycc(epi.k, rgb[0], rgb[1], rgb[2], Yv, cbv, crv);
            [[maybe_unused]] float cbs = cbv, crs = crv, cbo = 0.f, cro = 0.f;
            if constexpr (C420 || C422) {   // left + right of the block's row: the partner is lane group g ^ 1
                cbs = hat_add_rn(cbv, __shfl_xor(cbv, 16));
                crs = hat_add_rn(crv, __shfl_xor(crv, 16));
            }
            if constexpr (C420) {           // the bottom row's sums come to the top row's lanes
                cbo = __shfl_xor(cbs, 32);
                cro = __shfl_xor(crs, 32);
            }
            if (ok && oy < epi.h_out && ox < epi.w_out) {
                yuv_store_luma(epi.d, epi.q, b, oy, ox, Yv);
                if constexpr (C420) {
                    if (g == 0 && oy + 1 < epi.h_out) yuv_store_chroma420(epi.d, epi.q, epi.k, b, py, px, cbs, cbo, crs, cro);
                } else if constexpr (C422) {
                    if (!(g & 1)) yuv_store_chroma422(epi.d, epi.q, epi.k, b, oy, px, cbs, crs);
                } else if constexpr (C444) {
                    yuv_store_chroma444(epi.d, epi.q, epi.k, b, oy, ox, cbv, crv);
                }
            }
        } else if constexpr (U8) {
            if (ok && oy < epi.h_out && ox < epi.w_out) {
                uint8_t* p = reinterpret_cast<uint8_t*>(outv) + (size_t)b * epi.bstride + (size_t)oy * epi.pitch + (size_t)ox * 3;
#pragma unroll
                for (int m = 0; m < 3; ++m) p[epi.bgr ? 2 - m : m] = (uint8_t)hat_unit_to_u8(rgb[m]);
            }
        } else {
            if (ok) {
                float* of = reinterpret_cast<float*>(outv) + (size_t)b * 3 * Ho * Wo + (size_t)oy * Wo + ox;
#pragma unroll
                for (int m = 0; m < 3; ++m) of[(size_t)m * Ho * Wo] = rgb[m];
            }
        }
    };

    // ---- one 16-pixel group with the fragments of variant v from global memory: lane column c16 is haloed pixel (hy, hx) ------
    auto slow_group = [&](int v, int hy, int hx) -> f32x4 {
        const bf16_t* wv = wpk + (size_t)v * F_VARIANT + lane * 8;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
        for (int ty = 0; ty < 5; ++ty) {   // (rolled: ten fragment loads in flight are enough for a few groups per border tile)
#pragma unroll
            for (int tx = 0; tx < 5; ++tx)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf8 a = __builtin_bit_cast(bf8, *reinterpret_cast<const u32x4*>(wv + ((ty * 5 + tx) * 2 + ks) * 512));
                    const bf8 bf = __builtin_bit_cast(bf8, *reinterpret_cast<const u32x4*>(smem + F_X_OFF + fold_x_addr(hy + ty - 2, hx + tx - 2, ks * 4 + g)));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf, acc, 0, 0, 0);
                }
        }
        return acc;
    };

    // The next tile's haloed input is fetched into registers BEFORE this tile's K loop and written to LDS after it.
    constexpr int NPIECE = F_HR * F_HC * 8, NIT = (NPIECE + F_THREADS - 1) / F_THREADS;
    u32x4 pv[NIT];
    auto fetch = [&](int t) {
        const int tc = min(t, ntiles - 1);
        const int ty0 = (tc / tiles_x) * F_TR, tx0 = (tc - (tc / tiles_x) * tiles_x) * F_TC;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = min(tid + it * F_THREADS, NPIECE - 1);
            const int hp = i >> 3, s = i & 7;
            const int hy = hp / F_HC, hx = hp - hy * F_HC;
            const int y = ty0 - F_HALO + hy, xx = tx0 - F_HALO + hx;
            const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
            const u32x4 v = *reinterpret_cast<const u32x4*>(xb + ((size_t)min(max(y, 0), H - 1) * W + min(max(xx, 0), W - 1)) * ldx + s * 8);
            pv[it] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
    };
    const int q4 = 4 * (wave >> 1), ch = wave & 1;   // this wave's rows q4 .. q4 + 3 and column half of the tile
    fetch(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty0 = (t / tiles_x) * F_TR, tx0 = (t - (t / tiles_x) * tiles_x) * F_TC;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * F_THREADS;
            if (i < NPIECE) {
                const int hp = i >> 3, hx = hp % F_HC;
                *reinterpret_cast<u32x4*>(smem + F_X_OFF + hp * 128 + (((i & 7) ^ ((hx >> 1) & 7)) << 4)) = pv[it];
            }
        }
        __syncthreads();   // (first tile: also publishes the weights)
        fetch(t + gridDim.x);   // in flight during the K loop (clamped to a valid tile past the end)

        // ---- main pass: interior weights from LDS ---------------------------------------------------------------------------
        const int px = tx0 + 16 * ch + c16;
        if (tx0 + 16 * ch < W) {   // (wave-uniform: W % 16 == 0, so a column half is inside or outside as a whole)
            f32x4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tx = 0; tx < 5; ++tx) {
                const int hx = 16 * ch + c16 + tx;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf8 rowf[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        rowf[i] = __builtin_bit_cast(bf8, *reinterpret_cast<const u32x4*>(smem + F_X_OFF + fold_x_addr(q4 + i, hx, ks * 4 + g)));
#pragma unroll
                    for (int ty = 0; ty < 5; ++ty) {
                        const bf8 a = __builtin_bit_cast(bf8, *reinterpret_cast<const u32x4*>(smem + ((ty * 5 + tx) * 2 + ks) * 1024 + lane * 16));
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, rowf[j + ty], acc[j], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // (left alone the scheduler hoists every tap column's reads above the first MFMA)
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int py = ty0 + q4 + j;
                finish(acc[j], bias0, py, px, py > 0 && py < H - 1 && px > 0 && px < W - 1);
            }
        }

        // ---- border pixels: one slow group per edge and column half, by the first six waves (workgroup-uniform conditions) -----
        const int rs_top = 1 + (H == 1 ? 2 : 0);   // the row state of row 0 (first; also last when H == 1)
        const bool has_top = ty0 == 0, has_bot = H > 1 && ty0 + F_TR >= H;      // (the last tile row holds row H - 1)
        const bool has_left = tx0 == 0, has_right = tx0 + F_TC >= W;
        if (wave < 4) {   // rows: wave 0, 1 the first row's column halves; wave 2, 3 the last row's
            const bool top = wave < 2;
            const int py = top ? 0 : H - 1, half = wave & 1;
            const int pxr = tx0 + 16 * half + c16;
            if ((top ? has_top : has_bot) && tx0 + 16 * half < W) {
                const int v = 3 * (top ? rs_top : 2);
                const f32x4 acc = slow_group(v, py - ty0 + F_HALO, 16 * half + c16 + F_HALO);
                finish(acc, *reinterpret_cast<const f32x4*>(bias + v * 16 + 4 * g), py, pxr, pxr > 0 && pxr < W - 1);
            }
        } else if (wave < 6) {   // columns: wave 4 the first column, wave 5 the last; lane c16 is row ty0 + c16
            const bool left = wave == 4;
            if (left ? has_left : has_right) {
                const int pxc = left ? 0 : W - 1, cs = left ? 1 : 2;
                const int py = ty0 + c16, hy = c16 + F_HALO, hx = pxc - tx0 + F_HALO;
                const int rs = (py == 0 ? 1 : 0) | (py == H - 1 ? 2 : 0);
                f32x4 acc = slow_group(cs, hy, hx);
                if (has_top) {
                    const f32x4 a2 = slow_group(3 * rs_top + cs, hy, hx);
                    if (py == 0) acc = a2;
                }
                if (has_bot) {
                    const f32x4 a2 = slow_group(3 * 2 + cs, hy, hx);
                    if (py == H - 1 && py != 0) acc = a2;
                }
                const int rsc = py < H ? rs : 0;   // (rows past the image read a valid variant and are not stored)
                finish(acc, *reinterpret_cast<const f32x4*>(bias + (3 * rsc + cs) * 16 + 4 * g), py, pxc, py < H);
            }
        }
        __syncthreads();   // every wave is done with the input tile before the next one overwrites it
    }
}

int fold_args_ok(const void* x, const void* wpk, const float* bias, int B, int H, int W, int ldx, int dtype) {
    if (!x || !wpk || !bias || B < 1 || H < 1 || W < 16 || W % 16 || ldx < 64 || ldx % 8) return HAT_EINVAL;
    if (H > (1 << 14) || W > (1 << 14)) return HAT_EINVAL;
    if (dtype != HAT_BF16) return HAT_EUNSUPPORTED;
    return (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpk) | reinterpret_cast<uintptr_t>(bias)) % 16 ? HAT_EINVAL : 0;
}

template <typename Epi>
int launch_fold(const void* x, const void* wpk, const float* bias, void* out, int B, int H, int W, int ldx, const Epi& epi, void* stream) {
    const int tiles_x = (W + F_TC - 1) / F_TC, tiles_y = (H + F_TR - 1) / F_TR, ntiles = tiles_x * tiles_y;
    int gx = 256 / B;   // persistent: gx x B workgroups, at most one per CU over the batch (B > 256: one per sample)
    if (gx < 1) gx = 1;
    if (gx > ntiles) gx = ntiles;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(upfold_kernel<Epi>), hipFuncAttributeMaxDynamicSharedMemorySize, F_LDS);
    if (e != hipSuccess) return (int)e;
    HAT_LAUNCH(upfold_kernel<Epi>, dim3(gx, B), dim3(F_THREADS), F_LDS, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const bf16_t*>(x),
               ldx, reinterpret_cast<const bf16_t*>(wpk), bias, out, H, W, tiles_x, ntiles, epi);
    return hat_check_launch();
}

}  // namespace

extern "C" int hat_upfold_to_planes(const void* x, const void* wpk, const float* bias, float* out, int32_t B, int32_t H, int32_t W,
                                    int32_t ldx, float out_scale, float mean_r, float mean_g, float mean_b, int32_t dtype, void* stream) {
    if (!out) return HAT_EINVAL;
    if (const int rc = fold_args_ok(x, wpk, bias, B, H, W, ldx, dtype)) return rc;
    return launch_fold(x, wpk, bias, out, B, H, W, ldx, FoldEpi{out_scale, {mean_r, mean_g, mean_b}}, stream);
}

// hat_conv's out_mode HAT_O_FOLD2_NCHW_F32: the planes form behind a HatConvDesc (what a forward plan records)
int hat_upfold_launch_desc(const HatConvDesc& d, hipStream_t s) {
    if (d.ksize != 5 || d.Cin != 64 || d.x_mode != HAT_X_NHWC_T || d.act != HAT_ACT_NONE || d.w_bstride != 0 || d.reserved0 != 0) return HAT_EINVAL;
    if (d.x0 || d.r1 || d.r2 || d.r2scale || d.colsum || d.ln_out || d.gap_out || d.n16_out) return HAT_EINVAL;
    return hat_upfold_to_planes(d.x, d.w, d.bias, reinterpret_cast<float*>(d.out), d.B, d.H, d.W, d.ldx, d.out_scale, d.mean[0], d.mean[1],
                                d.mean[2], d.dtype, s);
}

extern "C" int hat_upfold_to_u8(const void* x, const void* wpk, const float* bias, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride,
                                int32_t B, int32_t H, int32_t W, int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, float mean_r,
                                float mean_g, float mean_b, int32_t bgr, int32_t dtype, void* stream) {
    if (!dst || h_out < 1 || w_out < 1) return HAT_EINVAL;
    if (const int rc = fold_args_ok(x, wpk, bias, B, H, W, ldx, dtype)) return rc;
    if (h_out > 2 * H || w_out > 2 * W) return HAT_EINVAL;
    if (dst_pitch < 3 * (int64_t)w_out || (B > 1 && dst_bstride < dst_pitch * (int64_t)(h_out - 1) + 3 * (int64_t)w_out)) return HAT_EINVAL;
    return launch_fold(x, wpk, bias, dst, B, H, W, ldx,
                       FoldEpiU8{out_scale, {mean_r, mean_g, mean_b}, h_out, w_out, bgr ? 1 : 0, (long long)dst_pitch, (long long)dst_bstride}, stream);
}

extern "C" int hat_upfold_to_yuv(const void* x, const void* wpk, const float* bias, const HatYuvSurface* dst, int32_t B, int32_t H, int32_t W,
                                 int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, float mean_r, float mean_g, float mean_b,
                                 const float* from_rgb12, int32_t dtype, void* stream) {
    if (!from_rgb12) return HAT_EINVAL;
    if (const int rc = fold_args_ok(x, wpk, bias, B, H, W, ldx, dtype)) return rc;
    if (h_out > 2 * H || w_out > 2 * W || !hat_yuv_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;
    int rc = 0;
    yuv_dispatch(*dst, [&](auto L, auto q) {
        using T = typename decltype(L)::sample_t;
        using Epi = FoldEpiYuv<T, L.sx, L.sy, L.grey>;
        rc = launch_fold(x, wpk, bias, dst->y, B, H, W, ldx,
                         Epi{out_scale, {mean_r, mean_g, mean_b}, h_out, w_out, load_csc(from_rgb12), q, yuv_dst<T>(*dst)}, stream);
    });
    return rc;
}
