// hat_vgg.hip — SRVGGNetCompact's layer (srvgg_arch.py:33-53): a 3x3 conv to 64 channels with a per-channel slope on the negative
// side (PReLU; ReLU and LeakyReLU 0.1 as slope vectors), from 64-channel T rows (the body) or from the 3-channel fp32 frame (the
// first conv).  Contract: include/hat_mi355x.h "SRVGGNetCompact".  DESIGN.md 4.25.
//
// A resident-weight conv with the structure hat_conv3_tile.h describes (its schedule, launcher, block mapping and tile decode are that
// header's): the workgroup's slice is 72 KB of A fragments, all 64 outputs in bf16, 32 of them in fp32, whose 86 KB tile leaves no room
// for more.  Its own: the weights arrive in fragment order
// (packing.pack_vgg_conv), so their copy is linear; the epilogue applies slope[n]; bf16 rows leave as 16-byte stores
// (store_pair_bf16_if); the fp32 instantiation exists (hat_conv's products).
// Frame mode stages the three fp32 planes of the haloed tile (3.9 KB) and builds its one B fragment per tile row from them: lane
// (c16, g) holds k = 8 g + j = 9 ci + 3 ty + tx, a per-lane table of eight LDS offsets made once.
#include <type_traits>

#include "hat_conv3_tile.h"

namespace {

template <typename T> struct VggCfg {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int NTL = ES == 2 ? 4 : 2;                  // n-tiles a workgroup owns
    static constexpr int NSL = 4 / NTL;                          // output slices
    static constexpr int FRAGB = 64 * 8 * ES;                    // bytes of one A fragment
    static constexpr int ROWB = lds_row_elems(64, ES) * ES;      // bytes per haloed pixel in LDS: 160 / 272
    static constexpr int PPP = 64 * ES / 16;                     // 16-byte pieces per pixel row
    static constexpr int VEC = 16 / ES;
    static constexpr int lds(bool frame) { return (frame ? 1 : 18) * NTL * FRAGB + (frame ? 3 * C3_NPH * 4 : C3_NPH * ROWB); }
};
static_assert(VggCfg<bf16_t>::lds(false) == 125568 && VggCfg<float>::lds(false) == 161856 && VggCfg<float>::lds(false) <= HAT_LDS_MAX, "LDS budget");

template <typename T, bool FRAME>
__global__ __launch_bounds__(C3_NTHR) void vgg_conv_kernel(const HatVggConvDesc d, int nwps, int tiles_x, int tiles_y) {
    using M = MT<T>;
    using Cf = VggCfg<T>;
    using frag_t = typename M::frag_t;
    constexpr int NTL = Cf::NTL, NSL = Cf::NSL, KS = FRAME ? 1 : 18, WB = KS * NTL * Cf::FRAGB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = conv3_slice(NSL), wgi = conv3_wgi(NSL);
    const int H = d.H, W = d.W;
    const int ntiles = tiles_x * tiles_y * d.B;
    if (wgi >= ntiles) return;

    // ---- this slice's fragments -> LDS, once: [k-step][n-tile][lane][8], already in that order ----
    {
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(d.w) + (size_t)slice * WB);
        for (int i = tid; i < WB / 16; i += C3_NTHR) reinterpret_cast<u32x4*>(smem)[i] = wsrc[i];
    }
    char* const xs = smem + WB;
    const int r0 = 2 * wave;

    // The next tile's haloed input is fetched into registers BEFORE this tile's K loop and written to LDS after it.
    constexpr int NPIECE = FRAME ? 3 * C3_NPH : C3_NPH * Cf::PPP, NIT = (NPIECE + C3_NTHR - 1) / C3_NTHR;
    using piece_t = std::conditional_t<FRAME, float, u32x4>;
    piece_t pv[NIT];
    auto fetch = [&](int t) {
        const auto [bb, ty0, tx0] = conv3_tile(min(t, ntiles - 1), tiles_x, tiles_y);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = min(tid + it * C3_NTHR, NPIECE - 1);
            if constexpr (FRAME) {
                const int c = i / C3_NPH, hp = i - c * C3_NPH;
                const int hy = hp / C3_HW, hx = hp - hy * C3_HW;
                const int y = ty0 - 1 + hy, xx = tx0 - 1 + hx;
                const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
                const float v = reinterpret_cast<const float*>(d.x)[(((size_t)bb * 3 + c) * H + min(max(y, 0), H - 1)) * W + min(max(xx, 0), W - 1)];
                pv[it] = in ? v : 0.f;
            } else {
                const int hp = i / Cf::PPP, piece = i - hp * Cf::PPP;
                const int hy = hp / C3_HW, hx = hp - hy * C3_HW;
                const int y = ty0 - 1 + hy, xx = tx0 - 1 + hx;
                const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
                const T* xb = reinterpret_cast<const T*>(d.x) + (size_t)bb * H * W * d.ldx;
                const u32x4 v = *reinterpret_cast<const u32x4*>(xb + ((size_t)min(max(y, 0), H - 1) * W + min(max(xx, 0), W - 1)) * d.ldx + piece * Cf::VEC);
                pv[it] = in ? v : u32x4{0u, 0u, 0u, 0u};
            }
        }
    };
    f32x4 biasv[NTL], slopev[NTL];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        biasv[nt] = *reinterpret_cast<const f32x4*>(d.bias + (slice * NTL + nt) * 16 + 4 * g);
        slopev[nt] = *reinterpret_cast<const f32x4*>(d.slope + (slice * NTL + nt) * 16 + 4 * g);
    }
    // frame mode: where this lane's eight k = 8 g + j = 9 ci + 3 ty + tx sit in the staged planes, relative to its pixel (-1: k >= 27)
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * g + j, ci = k / 9, tap = k - 9 * ci;
        koff[j] = k < 27 ? ci * C3_NPH + (tap / 3) * C3_HW + tap % 3 : -1;
    }

    fetch(wgi);
    for (int t = wgi; t < ntiles; t += nwps) {
        const auto [bb, ty0, tx0] = conv3_tile(t, tiles_x, tiles_y);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * C3_NTHR;
            if (i < NPIECE) {
                if constexpr (FRAME) reinterpret_cast<float*>(xs)[i] = pv[it];
                else *reinterpret_cast<u32x4*>(xs + (i / Cf::PPP) * Cf::ROWB + (i % Cf::PPP) * 16) = pv[it];
            }
        }
        __syncthreads();   // (first tile: the weights too)
        fetch(t + nwps);   // in flight during the K loop (clamped to a valid tile past the end)

        f32x4 acc[NTL][2];
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) acc[nt][pt] = biasv[nt];
        auto lda = [&](int ks, int nt) { return M::load(reinterpret_cast<const T*>(smem + (ks * NTL + nt) * Cf::FRAGB) + lane * 8); };
        if constexpr (FRAME) {
            const float* xp = reinterpret_cast<const float*>(xs);
            frag_t b[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = koff[j] >= 0 ? xp[max(koff[j], 0) + (r0 + pt) * C3_HW + c16] : 0.f;
                    b[pt][j] = to_T<T>(v);
                }
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) {
                const frag_t a = lda(0, nt);
                acc[nt][0] = M::mma(a, b[0], acc[nt][0]);
                acc[nt][1] = M::mma(a, b[1], acc[nt][1]);
            }
        } else {
            // B fragment of (haloed row r0 + rr, tap column dx, channel half): lane (c16, g) -> pixel column c16 + dx, channels 32 half + 8 g
            auto ldb = [&](int rr, int dx, int half) {
                return M::load(reinterpret_cast<const T*>(xs + ((r0 + rr) * C3_HW + c16 + dx) * Cf::ROWB) + half * 32 + 8 * g);
            };
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    frag_t prev = ldb(0, dx, half);
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const frag_t nx = ldb(dy + 1, dx, half);
                        const int ks = (dy * 3 + dx) * 2 + half;
#pragma unroll
                        for (int nt = 0; nt < NTL; ++nt) {
                            const frag_t a = lda(ks, nt);
                            acc[nt][0] = M::mma(a, prev, acc[nt][0]);
                            acc[nt][1] = M::mma(a, nx, acc[nt][1]);
                        }
                        prev = nx;
                    }
                }
            }
        }
        // ---- epilogue: lane holds channels 16 (slice NTL + nt) + 4g .. +3 of pixel (r0 + pt, c16) ----
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int y = ty0 + r0 + pt, xx = tx0 + c16;
            const bool valid = y < H && xx < W;
            T* orow = reinterpret_cast<T*>(d.out) + (((size_t)bb * H + min(y, H - 1)) * W + min(xx, W - 1)) * d.ldo + slice * NTL * 16;
            f32x4 v[NTL];
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) {
                v[nt] = acc[nt][pt];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[nt][r] = v[nt][r] >= 0.f ? v[nt][r] : slopev[nt][r] * v[nt][r];
            }
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int nt = 0; nt < NTL; nt += 2) store_pair_bf16_if(orow, nt * 16, g, v[nt], v[nt + 1], valid);
            } else {
                if (valid) {
#pragma unroll
                    for (int nt = 0; nt < NTL; ++nt) Vec4<T>::store(orow + nt * 16 + 4 * g, v[nt]);
                }
            }
        }
        __syncthreads();   // every wave is done with the input tile before the next one overwrites it
    }
}

template <typename T, bool FRAME>
int vgg_launch(const HatVggConvDesc& d, hipStream_t s) {
    return conv3_launch(vgg_conv_kernel<T, FRAME>, VggCfg<T>::lds(FRAME), VggCfg<T>::NSL, d, s);
}

}  // namespace

extern "C" int hat_vgg_conv_tiles(int32_t B, int32_t H, int32_t W, int32_t dtype, int32_t* tiles, int32_t* wgs, int32_t* slices) {
    if (!tiles || !wgs || !slices || B < 1 || H < 1 || W < 1 || (dtype != HAT_BF16 && dtype != HAT_F32)) return HAT_EINVAL;
    return conv3_tiles_query(B, H, W, dtype == HAT_BF16 ? VggCfg<bf16_t>::NSL : VggCfg<float>::NSL, tiles, wgs, slices);
}

extern "C" int hat_vgg_conv(const HatVggConvDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatVggConvDesc& d = *dp;
    if (!d.x || !d.w || !d.bias || !d.slope || !d.out || d.out == d.x) return HAT_EINVAL;
    if (d.dtype != HAT_BF16 && d.dtype != HAT_F32) return HAT_EINVAL;
    if (d.B < 1 || d.H < 1 || d.W < 1) return HAT_EINVAL;
    const int vec = d.dtype == HAT_BF16 ? 8 : 4;   // elements per 16 bytes
    if (misaligned(d.w, 16) || misaligned(d.bias, 16) || misaligned(d.slope, 16) || misaligned(d.out, 16)) return HAT_EINVAL;
    if (misaligned(d.x, d.frame ? 4 : 16)) return HAT_EINVAL;
    if (d.ldo < 64 || d.ldo % vec) return HAT_EINVAL;
    if (!d.frame && (d.ldx < 64 || d.ldx % vec)) return HAT_EINVAL;
    if (conv3_ntiles(d.B, d.H, d.W) > C3_MAX_TILES) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.frame ? vgg_launch<bf16_t, true>(d, s) : vgg_launch<bf16_t, false>(d, s);
    return d.frame ? vgg_launch<float, true>(d, s) : vgg_launch<float, false>(d, s);
}
