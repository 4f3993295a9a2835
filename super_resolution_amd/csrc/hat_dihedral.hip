// hat_dihedral.hip — the eight flips / transposes of fp32 planes, with a scale and an optional accumulate: the data movement of
// the geometric self-ensemble (basicsr models/sr_model.py:132-178, "test_selfensemble": the network on the eight transforms of
// the input, every output transformed back, the mean of the eight).  Contract: include/hat_mi355x.h (hat_dihedral_f32).
//
// Member op = v | h << 1 | t << 2, applied in that order: v reverses W, h reverses H, t swaps H and W.  A source pixel (y, x)
// of an (H, W) plane therefore lands at (y', x') = (h ? H-1-y : y, v ? W-1-x : x) of an (H, W) plane without t, and at row x',
// column y' of a (W, H) plane with t.  The inverse undoes t first: without t it is the member itself (flips commute and are
// their own inverses); with t it is the member with v and h exchanged (ops 5 and 6, the quarter turns, are each other's
// inverses; 4 and 7 their own).  So the host folds `inverse` into the two flip flags and the kernels know forward maps only.
#include "hat_common.h"

namespace {

constexpr int TILE = 64;   // a block moves a TILE x TILE tile of one plane with 256 threads = 4 waves: 16 rows per wave

// value written for source value s: (accumulate ? dst : 0) + alpha * s, product and sum each rounded to fp32 on their own, so
// the result is the same bits as the unfused torch expression for every alpha.  The pragma is what keeps it so: without it hipcc
// contracts the two into one v_fmac_f32 (its default fp-contract), also through __fmul_rn / __fadd_rn.
__device__ __forceinline__ float dihedral_value(float base, float alpha, float s) {
#pragma clang fp contract(off)
    const float p = alpha * s;
    return base + p;
}

// Members without t.  Thread (tx, ty) writes dst columns x0 + tx of rows y0 + ty, + 4, ...: a wave stores one contiguous
// 256-byte row segment and loads one contiguous row segment of the source (ascending or, with fx, descending addresses over
// the lanes: the same cache lines either way).  No LDS.
__global__ __launch_bounds__(256) void dihedral_flip_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int fx,
                                                            int fy, float alpha, int accumulate) {
    const int xd = blockIdx.x * TILE + threadIdx.x;
    if (xd >= W) return;
    const size_t plane = (size_t)H * W, pofs = (size_t)blockIdx.z * plane;
    const int xs = fx ? W - 1 - xd : xd;
    const int y0 = blockIdx.y * TILE;
#pragma unroll 4
    for (int r = threadIdx.y; r < TILE; r += 4) {
        const int yd = y0 + r;
        if (yd >= H) break;
        const int ys = fy ? H - 1 - yd : yd;
        float* o = dst + pofs + (size_t)yd * W + xd;
        *o = dihedral_value(accumulate ? *o : 0.0f, alpha, src[pofs + (size_t)ys * W + xs]);
    }
}

// Members with t, through an LDS tile.  The block takes the source tile rows [y0, y0 + 64) x columns [x0, x0 + 64): wave ty loads
// row segments (lane tx = column x0 + tx, 256 contiguous bytes) into tile[row][column]; after the barrier it reads
// tile[tx][row'] — the transposed access — and stores destination row segments (lane tx = destination column, again 256
// contiguous bytes).  The flips are applied on the destination side: the destination of source (y, x) is row x' = fx ? W-1-x : x,
// column y' = fy ? H-1-y : y of the (W, H) plane, so a flipped axis mirrors the tile's position and reverses the lanes, and a
// wave still stores whole contiguous row segments.  Ragged edges: loads and stores outside the plane are skipped (the LDS
// cells they would have filled are never read, because the same bounds guard the store).
//
// LDS bank rule relied on (cdna_hip_programming.md, "LDS", bank structure): for ds_read_b32 and every ds_write the bank of byte
// address a is (a / 4) % 32, and a wave64 access is served as its two 32-lane halves: only lanes of one half can conflict.
// With a row pitch of TILE + 1 = 65 dwords the write tile[r][tx] hits bank (65 r + tx) % 32 = (r + tx) % 32 and the transposed read
// tile[tx][c] hits bank (65 tx + c) % 32 = (tx + c) % 32: in both, the 32 lanes of a half (32 consecutive tx) fall on 32 different
// banks.  Unpadded (pitch 64) the transposed read would put all 32 lanes of a half on one bank: a 32-way conflict.
__global__ __launch_bounds__(256) void dihedral_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                                 int fx, int fy, float alpha, int accumulate) {
    __shared__ float tile[TILE][TILE + 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const size_t pofs = (size_t)blockIdx.z * ((size_t)H * W);
    if (x0 + tx < W) {
#pragma unroll 4
        for (int r = ty; r < TILE; r += 4) {
            if (y0 + r >= H) break;
            tile[r][tx] = src[pofs + (size_t)(y0 + r) * W + x0 + tx];
        }
    }
    __syncthreads();
    // destination plane: W rows of H floats.  Lane tx holds source row ys = y0 + tx, i.e. destination column fy ? H-1-ys : ys;
    // loop index r is source column xs = x0 + r, i.e. destination row fx ? W-1-xs : xs
    const int ys = y0 + tx;
    if (ys >= H) return;
    const int cd = fy ? H - 1 - ys : ys;
#pragma unroll 4
    for (int r = ty; r < TILE; r += 4) {
        const int xs = x0 + r;
        if (xs >= W) break;
        const int rd = fx ? W - 1 - xs : xs;
        float* o = dst + pofs + (size_t)rd * H + cd;
        *o = dihedral_value(accumulate ? *o : 0.0f, alpha, tile[tx][r]);
    }
}

}  // namespace

extern "C" int hat_dihedral_f32(const float* src, float* dst, int32_t planes, int32_t H, int32_t W, int32_t op, int32_t inverse,
                                float alpha, int32_t accumulate, void* stream) {
    if (!src || !dst || op < 0 || op > 7 || planes < 1 || H < 1 || W < 1) return HAT_EINVAL;
    // grid limits: planes on grid z, tiles of either axis on grid x / y (a transposing member exchanges the axes)
    constexpr int64_t MAX_SIDE = 65535ll * TILE;
    if (planes > 65535 || H > MAX_SIDE || W > MAX_SIDE) return HAT_EINVAL;
    const uint64_t bytes = (uint64_t)planes * (uint64_t)H * (uint64_t)W * sizeof(float);
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s < d + bytes && d < s + bytes) return HAT_EINVAL;   // the ranges overlap (in place included): a tile would read written cells
    const int v = op & 1, h = (op >> 1) & 1, t = (op >> 2) & 1;
    const int fx = (inverse && t) ? h : v, fy = (inverse && t) ? v : h;
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, planes), block(TILE, 4);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (t)
        HAT_LAUNCH(dihedral_transpose_kernel, grid, block, 0, st, src, dst, H, W, fx, fy, alpha, accumulate ? 1 : 0);
    else
        HAT_LAUNCH(dihedral_flip_kernel, grid, block, 0, st, src, dst, H, W, fx, fy, alpha, accumulate ? 1 : 0);
    return hat_check_launch();
}
