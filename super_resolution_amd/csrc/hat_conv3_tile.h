// hat_conv3_tile.h — what the 3x3 convs with RESIDENT weights share: hat_conv64r.hip (the Upsample and 64 -> 64 convs behind
// hat_conv), hat_vgg.hip (SRVGGNetCompact's layer) and hat_rrdb.hip (RRDBNet's dense-block conv).  DESIGN.md 4.28.
//
// The structure, once: a persistent workgroup of 8 waves owns one slice of the output channels, keeps that slice's MFMA A fragments
// in LDS for its whole life and walks 16 x 16 tiles.  The 18 x 18 haloed input tile (rows of lds_row_elems(64, ES) elements:
// conflict-free fragment reads) is resident beside the weights; the next tile's (or chunk's) is fetched into registers BEFORE the K
// loop and written to LDS after it, so there is no barrier inside the K loop.  A wave owns two tile rows x all its channel tiles and
// sweeps the tap ROWS for a fixed (tap column, channel half): the input-row fragment tile row 1 uses for tap row dy is the one tile
// row 0 needs for dy + 1, so 4 row fragments feed 6 (tap row, tile row) pairs.
//
// Here: the geometry, the schedule and the launcher (host), the block mapping and the tile decode (device).  Fetch, put and sweep stay
// written out in each kernel: as shared helpers they compiled to other schedules and every kernel left its timing spread, two of
// them slower.
#pragma once
#include "hat_common.h"

namespace {

constexpr int C3_T = 16, C3_WAVES = 8, C3_HW = C3_T + 2, C3_NPH = C3_HW * C3_HW, C3_NTHR = C3_WAVES * 64;   // 18 x 18 = 324 haloed pixels
constexpr long long C3_MAX_TILES = 1LL << 30;   // the kernels walk tiles with int arithmetic: t + nwps (nwps <= 256) must not overflow

inline bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline long long conv3_ntiles(int B, int H, int W) { return (long long)((W + C3_T - 1) / C3_T) * ((H + C3_T - 1) / C3_T) * B; }

// groups of 8 workgroups per slice: 256 workgroups on a large frame (32 / nsl groups), no idle ones on a small
inline int conv3_groups(int nsl, long long ntiles) {
    int m = 32 / nsl;
    if (m < 1) m = 1;
    while (m > 1 && 8LL * (m - 1) >= ntiles) --m;
    return m;
}

// what hat_vgg_conv_tiles and hat_rdb_conv_tiles report, after their own argument checks
inline int conv3_tiles_query(int B, int H, int W, int nsl, int32_t* tiles, int32_t* wgs, int32_t* slices) {
    const long long nt = conv3_ntiles(B, H, W);
    if (nt > C3_MAX_TILES) return HAT_EINVAL;
    *tiles = (int32_t)nt;
    *wgs = 8 * conv3_groups(nsl, nt);
    *slices = nsl;
    return 0;
}

// kern(d, nwps, tiles_x, tiles_y, extra...) on 8 nsl m workgroups.  hat_vgg_conv and hat_rdb_conv refuse more than C3_MAX_TILES tiles
// before they come here; hat_conv64r_launch takes what hat_conv has accepted and, as before, makes no check of its own.
template <typename K, typename D, typename... X>
int conv3_launch(K kern, int lds, int nsl, const D& d, hipStream_t s, X... extra) {
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
    }
    const int tiles_x = (d.W + C3_T - 1) / C3_T, tiles_y = (d.H + C3_T - 1) / C3_T;
    const int m = conv3_groups(nsl, conv3_ntiles(d.B, d.H, d.W));
    HAT_LAUNCH(kern, dim3(8 * nsl * m), dim3(C3_NTHR), lds, s, d, 8 * m, tiles_x, tiles_y, extra...);
    return hat_check_launch();
}

// Workgroups are dealt round-robin to the 8 XCDs: the nsl slice-workgroups that walk the same tiles sit on one XCD (consecutive
// groups of 8 block indices), so the input tile comes from HBM once and from that XCD's L2 nsl - 1 times.
__device__ __forceinline__ int conv3_slice(int nsl) { return ((int)blockIdx.x >> 3) % nsl; }
__device__ __forceinline__ int conv3_wgi(int nsl) { return (((int)blockIdx.x >> 3) / nsl) * 8 + ((int)blockIdx.x & 7); }

struct Conv3Tile { int bb, ty0, tx0; };   // image, top-left pixel
__device__ __forceinline__ Conv3Tile conv3_tile(int t, int tiles_x, int tiles_y) {
    const int bb = t / (tiles_x * tiles_y), tr = t - bb * tiles_x * tiles_y;
    return {bb, (tr / tiles_x) * C3_T, (tr - (tr / tiles_x) * tiles_x) * C3_T};
}

}  // namespace
