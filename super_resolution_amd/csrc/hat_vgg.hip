// hat_vgg.hip — SRVGGNetCompact's layer (srvgg_arch.py:33-53): a 3x3 conv to 64 channels with a per-channel slope on the negative
// side (PReLU; ReLU and LeakyReLU 0.1 as slope vectors), from 64-channel T rows (the body) or from the 3-channel fp32 frame (the
// first conv).  Contract: include/hat_mi355x.h "SRVGGNetCompact".  DESIGN.md 4.25.
//
// The structure is hat_conv64r.hip's: a persistent workgroup of 8 waves keeps the MFMA A fragments of its output slice in LDS (72 KB:
// all 64 outputs in bf16, 32 of them in fp32, whose 86 KB tile leaves no room for more), the 18 x 18 haloed input tile is resident
// beside them, the next tile's is fetched into registers before the K loop and written after it (no barrier inside the K loop), a wave
// owns two tile rows and sweeps the tap rows for a fixed (tap column, channel half) so that four row fragments feed six (tap row,
// tile row) pairs.  What differs: the weights arrive in fragment order (packing.pack_vgg_conv), so their copy is linear; the epilogue
// applies slope[n]; bf16 rows leave as 16-byte stores (store_pair_bf16_if); the fp32 instantiation exists (hat_conv's products).
// Frame mode stages the three fp32 planes of the haloed tile (3.9 KB) and builds its one B fragment per tile row from them: lane
// (c16, g) holds k = 8 g + j = 9 ci + 3 ty + tx, a per-lane table of eight LDS offsets made once.
#include <type_traits>

#include "hat_common.h"

namespace {

constexpr int V_T = 16, V_WAVES = 8, V_HW = V_T + 2, V_NPH = V_HW * V_HW, V_NTHR = V_WAVES * 64;
constexpr long long V_MAX_TILES = 1LL << 30;   // the kernel walks tiles with int arithmetic: t + nwps (nwps <= 256) must not overflow

template <typename T> struct VggCfg {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int NTL = ES == 2 ? 4 : 2;                  // n-tiles a workgroup owns
    static constexpr int NSL = 4 / NTL;                          // output slices
    static constexpr int FRAGB = 64 * 8 * ES;                    // bytes of one A fragment
    static constexpr int ROWB = lds_row_elems(64, ES) * ES;      // bytes per haloed pixel in LDS: 160 / 272
    static constexpr int PPP = 64 * ES / 16;                     // 16-byte pieces per pixel row
    static constexpr int VEC = 16 / ES;
    static constexpr int lds(bool frame) { return (frame ? 1 : 18) * NTL * FRAGB + (frame ? 3 * V_NPH * 4 : V_NPH * ROWB); }
};
static_assert(VggCfg<bf16_t>::lds(false) == 125568 && VggCfg<float>::lds(false) == 161856 && VggCfg<float>::lds(false) <= HAT_LDS_MAX, "LDS budget");

// groups of 8 workgroups per slice (hat_conv64r_launch's rule): 256 workgroups on a large frame, no idle ones on a small
inline int vgg_groups(int nsl, long long ntiles) {
    int m = 32 / nsl;
    while (m > 1 && 8LL * (m - 1) >= ntiles) --m;
    return m;
}

template <typename T, bool FRAME>
__global__ __launch_bounds__(V_NTHR) void vgg_conv_kernel(const HatVggConvDesc d, int nwps, int tiles_x, int tiles_y) {
    using M = MT<T>;
    using Cf = VggCfg<T>;
    using frag_t = typename M::frag_t;
    constexpr int NTL = Cf::NTL, NSL = Cf::NSL, KS = FRAME ? 1 : 18, WB = KS * NTL * Cf::FRAGB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // as in conv64r_kernel: the NSL slice-workgroups that walk the same tiles sit on one XCD
    const int slice = ((int)blockIdx.x >> 3) % NSL;
    const int wgi = (((int)blockIdx.x >> 3) / NSL) * 8 + ((int)blockIdx.x & 7);
    const int H = d.H, W = d.W;
    const int ntiles = tiles_x * tiles_y * d.B;
    if (wgi >= ntiles) return;

    // ---- this slice's fragments -> LDS, once: [k-step][n-tile][lane][8], already in that order ----
    {
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(d.w) + (size_t)slice * WB);
        for (int i = tid; i < WB / 16; i += V_NTHR) reinterpret_cast<u32x4*>(smem)[i] = wsrc[i];
    }
    char* const xs = smem + WB;
    const int r0 = 2 * wave;

    // The next tile's haloed input is fetched into registers BEFORE this tile's K loop and written to LDS after it.
    constexpr int NPIECE = FRAME ? 3 * V_NPH : V_NPH * Cf::PPP, NIT = (NPIECE + V_NTHR - 1) / V_NTHR;
    using piece_t = std::conditional_t<FRAME, float, u32x4>;
    piece_t pv[NIT];
    auto fetch = [&](int t) {
        const int tc = min(t, ntiles - 1);
        const int bb = tc / (tiles_x * tiles_y), tr = tc - bb * tiles_x * tiles_y;
        const int ty0 = (tr / tiles_x) * V_T, tx0 = (tr - (tr / tiles_x) * tiles_x) * V_T;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = min(tid + it * V_NTHR, NPIECE - 1);
            if constexpr (FRAME) {
                const int c = i / V_NPH, hp = i - c * V_NPH;
                const int hy = hp / V_HW, hx = hp - hy * V_HW;
                const int y = ty0 - 1 + hy, xx = tx0 - 1 + hx;
                const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
                const float v = reinterpret_cast<const float*>(d.x)[(((size_t)bb * 3 + c) * H + min(max(y, 0), H - 1)) * W + min(max(xx, 0), W - 1)];
                pv[it] = in ? v : 0.f;
            } else {
                const int hp = i / Cf::PPP, piece = i - hp * Cf::PPP;
                const int hy = hp / V_HW, hx = hp - hy * V_HW;
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
        koff[j] = k < 27 ? ci * V_NPH + (tap / 3) * V_HW + tap % 3 : -1;
    }

    fetch(wgi);
    for (int t = wgi; t < ntiles; t += nwps) {
        const int bb = t / (tiles_x * tiles_y), tr = t - bb * tiles_x * tiles_y;
        const int ty0 = (tr / tiles_x) * V_T, tx0 = (tr - (tr / tiles_x) * tiles_x) * V_T;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * V_NTHR;
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
                    const float v = koff[j] >= 0 ? xp[max(koff[j], 0) + (r0 + pt) * V_HW + c16] : 0.f;
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
                return M::load(reinterpret_cast<const T*>(xs + ((r0 + rr) * V_HW + c16 + dx) * Cf::ROWB) + half * 32 + 8 * g);
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
int vgg_launch(const HatVggConvDesc& d, int tiles_x, int tiles_y, hipStream_t s) {
    using Cf = VggCfg<T>;
    auto kern = vgg_conv_kernel<T, FRAME>;
    constexpr int lds = Cf::lds(FRAME);
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
    }
    const int m = vgg_groups(Cf::NSL, (long long)tiles_x * tiles_y * d.B);
    HAT_LAUNCH(kern, dim3(8 * Cf::NSL * m), dim3(V_NTHR), lds, s, d, 8 * m, tiles_x, tiles_y);
    return hat_check_launch();
}

inline bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int hat_vgg_conv_tiles(int32_t B, int32_t H, int32_t W, int32_t dtype, int32_t* tiles, int32_t* wgs, int32_t* slices) {
    if (!tiles || !wgs || !slices || B < 1 || H < 1 || W < 1 || (dtype != HAT_BF16 && dtype != HAT_F32)) return HAT_EINVAL;
    const long long nt = (long long)((W + V_T - 1) / V_T) * ((H + V_T - 1) / V_T) * B;
    if (nt > V_MAX_TILES) return HAT_EINVAL;
    const int nsl = dtype == HAT_BF16 ? VggCfg<bf16_t>::NSL : VggCfg<float>::NSL;
    *tiles = (int32_t)nt;
    *wgs = 8 * vgg_groups(nsl, nt);
    *slices = nsl;
    return 0;
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
    const int tiles_x = (d.W + V_T - 1) / V_T, tiles_y = (d.H + V_T - 1) / V_T;
    if ((long long)tiles_x * tiles_y * d.B > V_MAX_TILES) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.dtype == HAT_BF16) return d.frame ? vgg_launch<bf16_t, true>(d, tiles_x, tiles_y, s) : vgg_launch<bf16_t, false>(d, tiles_x, tiles_y, s);
    return d.frame ? vgg_launch<float, true>(d, tiles_x, tiles_y, s) : vgg_launch<float, false>(d, tiles_x, tiles_y, s);
}
