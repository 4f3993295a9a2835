// hat_rrdb.hip — one 3x3 conv of RRDBNet's residual dense block (rrdbnet_arch.py:21-39) on DENSE ROWS: the block's input and its
// four grown maps share one (B,H,W,ldx) buffer, conv k reads channels [0, Cin) and stores its 32 outputs at channel Cin of the same
// buffer, so torch.cat is never made.  Conv 5 (Cin 192, 64 outputs) carries the residual arithmetic of :39 and :62 on an fp32 stream.
// Contract: include/hat_mi355x.h "RRDBNet".  DESIGN.md 4.26.
//
// A resident-weight conv with the structure hat_conv3_tile.h describes (its schedule, launcher, block mapping and tile decode are that
// header's): the workgroup's slice is the A fragments of 32 outputs.  The fetch, put and K sweep are written out here: as helpers
// shared with the other two kernels they compiled to other schedules and the layers ran up to 9 % slower.
// Its own besides is the depth.  Weights and a full-depth haloed tile never fit together (table below), so the weights stay and the INPUT is walked in channel chunks of 64 (the last one 32 wide where Cin is no
// multiple of 64): one chunk of the haloed tile is resident (324 px x 160 B), the next chunk (of this tile, or the first of the next
// tile) is fetched into registers before the chunk's MFMAs and written after them.  There is no barrier inside a chunk's K loop; two
// per chunk around the LDS write.  Conv 5 runs as two 32-output slices whose workgroups share an XCD, as hat_vgg_conv's fp32 slices do.
//
//   Cin   weights (9 Cin x 32 x 2 B)   + chunk 51,840 B   = LDS per workgroup      (full-depth tile: 324 px x lds_row(Cin) B)
//    64         36,864                                        88,704                 51,840
//    96         55,296                                       107,136                 72,576
//   128         73,728                                       125,568                 98,496
//   160         92,160                                       144,000                119,232
//   192        110,592 per slice                             162,432                134,784
//
// Reads and writes of one launch never share a byte: every 16-byte load covers 8 channels below Cin (a chunk ends at Cin, a multiple
// of 32), every store covers channels at or above the output offset, which hat_rdb_conv requires to be >= Cin when out == x.
#include "hat_conv3_tile.h"

namespace {

constexpr int R_NTL = 2;                       // n-tiles a workgroup owns: 32 outputs
constexpr int R_FRAGB = 64 * 8 * 2;            // bytes of one bf16 A fragment
constexpr int R_ROWB = lds_row_elems(64, 2) * 2;   // bytes per haloed pixel of a chunk in LDS: 160
constexpr int R_CHUNKB = C3_NPH * R_ROWB;       // 51,840

constexpr int rdb_wb(int cin) { return 9 * (cin / 32) * R_NTL * R_FRAGB; }   // resident weight bytes of a workgroup
constexpr int rdb_lds(int cin) { return rdb_wb(cin) + R_CHUNKB; }
static_assert(R_ROWB == 160 && R_CHUNKB == 51840, "chunk image");
static_assert(rdb_lds(64) == 88704 && rdb_lds(96) == 107136 && rdb_lds(128) == 125568 && rdb_lds(160) == 144000 && rdb_lds(192) == 162432, "LDS budget per layer");
static_assert(rdb_lds(192) <= HAT_LDS_MAX, "conv 5: one 32-output slice and one 64-channel chunk");
static_assert(2 * rdb_wb(192) > HAT_LDS_MAX, "conv 5's 64 outputs cannot be resident in one workgroup: two slices");
static_assert(rdb_wb(128) + C3_NPH * lds_row_elems(128, 2) * 2 > HAT_LDS_MAX, "convs 3-5: no full-depth tile beside the weights");

template <int CIN>
__global__ __launch_bounds__(C3_NTHR) void rdb_conv_kernel(const HatRdbConvDesc d, int nwps, int tiles_x, int tiles_y) {
    using M = MT<bf16_t>;
    using frag_t = typename M::frag_t;
    constexpr bool LAST = CIN == 192;
    constexpr int NSL = LAST ? 2 : 1, WB = rdb_wb(CIN), NCH = (CIN + 63) / 64;
    constexpr int NIT = (C3_NPH * 8 + C3_NTHR - 1) / C3_NTHR;   // 16-byte pieces of a 64-channel chunk per thread: 6
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = conv3_slice(NSL), wgi = conv3_wgi(NSL);
    const int H = d.H, W = d.W;
    const int ntiles = tiles_x * tiles_y * d.B;
    if (wgi >= ntiles) return;

    // ---- this slice's fragments -> LDS, once: [k-step = 9 (channel / 32) + tap][n-tile][lane][8], already in that order ----
    {
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(d.w) + (size_t)slice * WB);
        for (int i = tid; i < WB / 16; i += C3_NTHR) reinterpret_cast<u32x4*>(smem)[i] = wsrc[i];
    }
    char* const xs = smem + WB;
    const int r0 = 2 * wave;
    const bf16_t* const xg = reinterpret_cast<const bf16_t*>(d.x);

    // Chunk c of tile t -> registers.  ppp: 16-byte pieces per pixel of the chunk (8, or 4 for a 32-wide last chunk); no piece
    // reaches channel CIN or beyond.
    u32x4 pv[NIT];
    auto fetch = [&](int t, int c) {
        const int ppp = (c == NCH - 1 && CIN % 64) ? 4 : 8, npiece = C3_NPH * ppp;
        const auto [bb, ty0, tx0] = conv3_tile(min(t, ntiles - 1), tiles_x, tiles_y);
        const bf16_t* xb = xg + (size_t)bb * H * W * d.ldx + c * 64;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (it * C3_NTHR >= npiece) break;
            const int i = min(tid + it * C3_NTHR, npiece - 1);
            const int hp = i / ppp, piece = i - hp * ppp;
            const int hy = hp / C3_HW, hx = hp - hy * C3_HW;
            const int y = ty0 - 1 + hy, xx = tx0 - 1 + hx;
            const bool in = y >= 0 && y < H && xx >= 0 && xx < W;
            const u32x4 v = *reinterpret_cast<const u32x4*>(xb + ((size_t)min(max(y, 0), H - 1) * W + min(max(xx, 0), W - 1)) * d.ldx + piece * 8);
            pv[it] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto put = [&](int c) {
        const int ppp = (c == NCH - 1 && CIN % 64) ? 4 : 8, npiece = C3_NPH * ppp;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * C3_NTHR;
            if (i < npiece) *reinterpret_cast<u32x4*>(xs + (i / ppp) * R_ROWB + (i % ppp) * 16) = pv[it];
        }
    };
    f32x4 biasv[R_NTL];
#pragma unroll
    for (int nt = 0; nt < R_NTL; ++nt) biasv[nt] = *reinterpret_cast<const f32x4*>(d.bias + (slice * R_NTL + nt) * 16 + 4 * g);
    const float slope = d.slope, beta1 = d.beta1, beta2 = d.beta2;

    fetch(wgi, 0);
    for (int t = wgi; t < ntiles; t += nwps) {
        const auto [bb, ty0, tx0] = conv3_tile(t, tiles_x, tiles_y);
        f32x4 acc[R_NTL][2];
#pragma unroll
        for (int nt = 0; nt < R_NTL; ++nt)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) acc[nt][pt] = biasv[nt];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            put(c);
            __syncthreads();   // (first chunk of the first tile: the weights too)
            // in flight during the chunk's K loop: the next chunk of this tile, or the first of the next tile (clamped past the end)
            if (c + 1 < NCH) fetch(t, c + 1);
            else fetch(t + nwps, 0);
            const int nh = (c == NCH - 1 && CIN % 64) ? 1 : 2;   // 32-channel halves of the chunk
            auto lda = [&](int ks, int nt) { return M::load(reinterpret_cast<const bf16_t*>(smem + (ks * R_NTL + nt) * R_FRAGB) + lane * 8); };
            // B fragment of (haloed row r0 + rr, tap column dx, half): lane (c16, g) -> pixel column c16 + dx, channels 32 half + 8 g
            auto ldb = [&](int rr, int dx, int half) {
                return M::load(reinterpret_cast<const bf16_t*>(xs + ((r0 + rr) * C3_HW + c16 + dx) * R_ROWB) + half * 32 + 8 * g);
            };
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (half >= nh) break;
                    frag_t prev = ldb(0, dx, half);
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const frag_t nx = ldb(dy + 1, dx, half);
                        const int ks = (2 * c + half) * 9 + dy * 3 + dx;
#pragma unroll
                        for (int nt = 0; nt < R_NTL; ++nt) {
                            const frag_t a = lda(ks, nt);
                            acc[nt][0] = M::mma(a, prev, acc[nt][0]);
                            acc[nt][1] = M::mma(a, nx, acc[nt][1]);
                        }
                        prev = nx;
                    }
                }
            }
            __syncthreads();   // every wave is done with the chunk before the next one overwrites it
        }
        // ---- epilogue: lane holds channels 16 (slice R_NTL + nt) + 4g .. +3 of pixel (r0 + pt, c16) ----
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int y = ty0 + r0 + pt, xx = tx0 + c16;
            const bool valid = y < H && xx < W;
            const size_t p = ((size_t)bb * H + min(y, H - 1)) * W + min(xx, W - 1);
            bf16_t* orow = reinterpret_cast<bf16_t*>(d.out) + p * d.ldo + d.out_off + slice * 32;
            f32x4 v[R_NTL];
#pragma unroll
            for (int nt = 0; nt < R_NTL; ++nt) {
                v[nt] = acc[nt][pt];
                if constexpr (LAST) {
                    const size_t so = p * 64 + slice * 32 + nt * 16 + 4 * g;
                    f32x4 r = {0.f, 0.f, 0.f, 0.f};
                    if (d.r1) r = *reinterpret_cast<const f32x4*>(d.r1 + so);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[nt][q] = beta1 * v[nt][q] + r[q];
                    if (d.r2) {
                        r = *reinterpret_cast<const f32x4*>(d.r2 + so);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[nt][q] = beta2 * v[nt][q] + r[q];
                    }
                    if (valid) *reinterpret_cast<f32x4*>(d.s_out + so) = v[nt];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[nt][q] = v[nt][q] >= 0.f ? v[nt][q] : slope * v[nt][q];
                }
            }
            store_pair_bf16_if(orow, 0, g, v[0], v[1], valid);
        }
    }
}

template <int CIN>
int rdb_launch(const HatRdbConvDesc& d, hipStream_t s) {
    return conv3_launch(rdb_conv_kernel<CIN>, rdb_lds(CIN), CIN == 192 ? 2 : 1, d, s);
}
inline bool rdb_cin_ok(int cin) { return cin >= 64 && cin <= 192 && cin % 32 == 0; }

}  // namespace

extern "C" int hat_rdb_conv_tiles(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t* tiles, int32_t* wgs, int32_t* slices) {
    if (!tiles || !wgs || !slices || B < 1 || H < 1 || W < 1 || !rdb_cin_ok(cin)) return HAT_EINVAL;
    return conv3_tiles_query(B, H, W, cin == 192 ? 2 : 1, tiles, wgs, slices);
}

extern "C" int hat_rdb_conv(const HatRdbConvDesc* dp, void* stream) {
    if (!dp) return HAT_EINVAL;
    const HatRdbConvDesc& d = *dp;
    if (!d.x || !d.w || !d.bias || !d.out) return HAT_EINVAL;
    if (d.dtype != HAT_BF16 && d.dtype != HAT_F32) return HAT_EINVAL;
    if (!rdb_cin_ok(d.cin) || d.cout != (d.cin == 192 ? 64 : 32)) return HAT_EINVAL;
    if (d.B < 1 || d.H < 1 || d.W < 1) return HAT_EINVAL;
    const int vec = d.dtype == HAT_BF16 ? 8 : 4;   // elements per 16 bytes
    if (misaligned(d.x, 16) || misaligned(d.w, 16) || misaligned(d.bias, 16) || misaligned(d.out, 16)) return HAT_EINVAL;
    if (d.ldx < d.cin || d.ldx % vec || d.out_off < 0 || d.out_off % vec || d.ldo % vec || (long long)d.ldo < (long long)d.out_off + d.cout) return HAT_EINVAL;
    if (d.out == d.x && (d.out_off < d.cin || d.ldo != d.ldx)) return HAT_EINVAL;   // in place: the stored slot lies beyond what is read
    if (d.cin == 192) {
        if (!d.s_out || (d.r2 && !d.r1)) return HAT_EINVAL;
        if (misaligned(d.s_out, 16) || misaligned(d.r1, 16) || misaligned(d.r2, 16)) return HAT_EINVAL;
    } else if (d.r1 || d.r2 || d.s_out) {
        return HAT_EINVAL;   // the fp32 stream belongs to conv 5
    }
    if (conv3_ntiles(d.B, d.H, d.W) > C3_MAX_TILES) return HAT_EINVAL;
    if (d.dtype != HAT_BF16) return HAT_EUNSUPPORTED;   // the fp32 compute path runs these layers on hat_conv
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (d.cin) {
        case 64: return rdb_launch<64>(d, s);
        case 96: return rdb_launch<96>(d, s);
        case 128: return rdb_launch<128>(d, s);
        case 160: return rdb_launch<160>(d, s);
        default: return rdb_launch<192>(d, s);
    }
}
