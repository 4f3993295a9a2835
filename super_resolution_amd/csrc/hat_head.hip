// hat_head.hip — hat_head_fused: conv_first, the patch-embed LayerNorm and the first block's norm1 in one launch
// (embed_dim 144, bf16).  Contract: include/hat_mi355x.h (HatHeadDesc).
//
// The three launches it replaces move the 144-channel fp32 map five times (conv writes f0; LN reads f0, writes t; LN reads
// t); here f0 and t are written once and never read.  Every value equals the three-launch result bit for bit:
//   conv   hat_conv's packed weights and k order: k = tap * 8 + ci, MFMA steps ks = 0, 1, 2 in that order (taps 0-3, 4-7, 8;
//          hat_conv's fourth step multiplies the zero padding of Kpad), the fp32 bias added behind them.
//   LN     ln_kernel's expressions in ln_kernel's order (hat_misc.hip).  There lane j of a pixel's 16 lanes owns the channel
//          quads j, j + 16, j + 32 and row_sum16 adds the 16 partial sums as the tree ((j, j+8), (j, j+4)), (j, j+2), (j, j+1).
//          Here the MFMA D layout gives lane group g of a pixel the quads 4 nt + g, nt < 9, i.e. ln_kernel's lanes j = 4 m + g,
//          m < 4: the first two tree levels are additions inside the lane, the last two cross the four lane groups.
//   GAP    a wave is one block of ln_kernel's partition: 16 consecutive pixels every LN_BLOCKS * 16, summed per pixel slot
//          over the trips and then over the 16 slots in order.
#include "hat_common.h"

namespace {

constexpr int HEAD_BLOCKS = 1024;   // = hat_layernorm_blocks(): chains (waves) per sample
constexpr int HEAD_WAVES = 4;       // chains per workgroup
constexpr int HC = 144, HNT = 9, HKS = 3;
constexpr int HLDW = lds_row_elems(HKS * 32, 2);   // LDS row stride of the weight image

struct HeadTile {   // one tile's input taps as loaded (clamped addresses), and which of them lie inside the image
    float v[HKS][3];
    unsigned ok;
};

// ln_kernel's LayerNorm of one pixel on the MFMA D layout; x[nt] = channels 16 nt + 4 g .. + 3.  gm / bt: LDS tables [144].
// Contraction is off and the two fused multiply-adds are spelled out: they are the ones ln_kernel compiles to (the squares of the
// variance are rounded before they are added there: its loop is vectorised into packed multiplies; eps and the affine are fma).
__device__ __forceinline__ void head_ln(const f32x4 (&x)[HNT], f32x4 (&o)[HNT], const float* gm, const float* bt, int g, float invC) {
#pragma clang fp contract(off)
    float P[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float s = 0.f;
        s += (x[m][0] + x[m][1]) + (x[m][2] + x[m][3]);
        s += (x[m + 4][0] + x[m + 4][1]) + (x[m + 4][2] + x[m + 4][3]);
        if (m == 0) s += (x[8][0] + x[8][1]) + (x[8][2] + x[8][3]);
        else s += (0.f + 0.f) + (0.f + 0.f);
        P[m] = s;
    }
    float s = (P[0] + P[2]) + (P[1] + P[3]);
    s += __shfl_xor(s, 32);
    s += __shfl_xor(s, 16);
    const float mean = s * invC;
    float Q[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float q = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float dlt = x[m][r] - mean; const float sq = dlt * dlt; q = q + sq; }
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float dlt = x[m + 4][r] - mean; const float sq = dlt * dlt; q = q + sq; }
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float dlt = x[8][r] - mean; const float sq = dlt * dlt; q = q + sq; }
        }
        Q[m] = q;
    }
    float q = (Q[0] + Q[2]) + (Q[1] + Q[3]);
    q += __shfl_xor(q, 32);
    q += __shfl_xor(q, 16);
    const float rstd = 1.0f / sqrtf(__builtin_fmaf(q, invC, 1e-5f));
#pragma unroll
    for (int nt = 0; nt < HNT; ++nt) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gm + nt * 16 + 4 * g);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bt + nt * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[nt][r] = __builtin_fmaf((x[nt][r] - mean) * rstd, gv[r], bv[r]);
    }
}

__global__ __launch_bounds__(HEAD_WAVES * 64) void head_fused_kernel(const HatHeadDesc d) {
    using M = MT<bf16_t>;
    __shared__ __attribute__((aligned(16))) bf16_t Ws[HC * HLDW];
    __shared__ __attribute__((aligned(16))) float tab[5][HC];      // bias, ln0 gamma / beta, ln1 gamma / beta
    __shared__ float red[HEAD_WAVES][16][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int b = blockIdx.y, blk = blockIdx.x * HEAD_WAVES + wave;
    const int H = d.H, W = d.W, npix = H * W;

    {   // the weight image: rows of 96 k's, 12 16-byte pieces each
        const bf16_t* wg = reinterpret_cast<const bf16_t*>(d.w);
        for (int i = tid; i < HC * 12; i += HEAD_WAVES * 64) {
            const int row = i / 12, pc = i - row * 12;
            *reinterpret_cast<u32x4*>(Ws + row * HLDW + pc * 8) = *reinterpret_cast<const u32x4*>(wg + (size_t)row * d.Kpad + pc * 8);
        }
        for (int i = tid; i < HC; i += HEAD_WAVES * 64) {
            tab[0][i] = d.bias[i];
            tab[1][i] = d.ln0_g[i];
            tab[2][i] = d.ln0_b[i];
            tab[3][i] = d.ln1_g[i];
            tab[4][i] = d.ln1_b[i];
        }
    }
    __syncthreads();

    const float* xb = d.x + (size_t)b * 3 * npix;
    float* f0b = d.f0 != nullptr ? d.f0 + (size_t)b * npix * HC : nullptr;
    float* tb = d.t + (size_t)b * npix * HC;
    bf16_t* nb = reinterpret_cast<bf16_t*>(d.n) + (size_t)b * npix * d.ldn;
    bf16_t* n16b = d.n16 != nullptr ? reinterpret_cast<bf16_t*>(d.n16) + (size_t)b * npix * 16 : nullptr;
    const float invC = 1.0f / (float)d.C;
    const float mean0 = d.mean[0], mean1 = d.mean[1], mean2 = d.mean[2], in_scale = d.in_scale;
    constexpr int STRIDE = HEAD_BLOCKS * 16;

    // the taps of tile p0: lane (c16, g) feeds k = 32 ks + 8 g + ci, i.e. tap 4 ks + g, channel ci, of pixel p0 + c16.  Every
    // load is unconditional on a clamped address (a tile past the image re-reads the last pixel: never used)
    auto fetch = [&](int p0, HeadTile& tl) {
        const int p = min(p0 + c16, npix - 1);
        const int y = p / W, x = p - y * W;
        tl.ok = 0u;
#pragma unroll
        for (int ks = 0; ks < HKS; ++ks) {
            const int tap = min(4 * ks + g, 8);
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (4 * ks + g < 9 && yy >= 0 && yy < H && xx >= 0 && xx < W) tl.ok |= 1u << ks;
            const size_t off = (size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) tl.v[ks][ci] = xb[(size_t)ci * npix + off];
        }
    };

    f32x4 gsum = {0.f, 0.f, 0.f, 0.f};
    HeadTile cur, nx1, nx2;
    int p0 = blk * 16;
    fetch(p0, cur);
    fetch(p0 + STRIDE, nx1);
    for (; p0 < npix; p0 += STRIDE) {
        fetch(p0 + 2 * STRIDE, nx2);   // two tiles ahead: its wait does not reach behind the previous tile's stores
        // ---- conv_first: (x - mean) * in_scale as bf16, zero padding applied after the shift (hat_conv, HAT_X_NCHW_F32_MEAN)
        f32x4 acc[HNT];
#pragma unroll
        for (int nt = 0; nt < HNT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < HKS; ++ks) {
            const bool in = (cur.ok >> ks) & 1u;
            M::frag_t bf = M::zero();
            bf[0] = to_T<bf16_t>(in ? (cur.v[ks][0] - mean0) * in_scale : 0.f);
            bf[1] = to_T<bf16_t>(in ? (cur.v[ks][1] - mean1) * in_scale : 0.f);
            bf[2] = to_T<bf16_t>(in ? (cur.v[ks][2] - mean2) * in_scale : 0.f);
#pragma unroll
            for (int nt = 0; nt < HNT; ++nt) acc[nt] = M::mma(M::load(Ws + (nt * 16 + c16) * HLDW + ks * 32 + 8 * g), bf, acc[nt]);
        }
        const int p = p0 + c16;
        const bool valid = p < npix;
        const size_t pc = (size_t)min(p, npix - 1);
#pragma unroll
        for (int nt = 0; nt < HNT; ++nt) {
            acc[nt] = acc[nt] + *reinterpret_cast<const f32x4*>(&tab[0][nt * 16 + 4 * g]);
            if (valid && f0b != nullptr) *reinterpret_cast<f32x4*>(f0b + pc * HC + nt * 16 + 4 * g) = acc[nt];
        }
        // ---- patch-embed LayerNorm -> t (fp32)
        f32x4 tv[HNT];
        head_ln(acc, tv, tab[1], tab[2], g, invC);
#pragma unroll
        for (int nt = 0; nt < HNT; ++nt)
            if (valid) *reinterpret_cast<f32x4*>(tb + pc * HC + nt * 16 + 4 * g) = tv[nt];
        // ---- norm1 of the first block -> n (bf16 rows), its compact copy and the pool of the stored values
        f32x4 nv[HNT];
        head_ln(tv, nv, tab[3], tab[4], g, invC);
        bf16_t* nrow = nb + pc * d.ldn;
#pragma unroll
        for (int nt = 0; nt + 1 < HNT; nt += 2) store_pair_bf16_if(nrow, nt * 16, g, nv[nt], nv[nt + 1], valid);
        if (valid) {
            Vec4<bf16_t>::store(nrow + 128 + 4 * g, nv[8]);
            if (n16b != nullptr) Vec4<bf16_t>::store(n16b + pc * 16 + 4 * g, nv[0]);
            if (4 * g < d.gap_c) gsum += as_stored<bf16_t>(nv[0]);
        }
        cur = nx1;
        nx1 = nx2;
    }
    if (d.gap_partial != nullptr) {   // ln_kernel's reduction over the 16 pixel slots, in order
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][c16][4 * g + r] = gsum[r];
        __syncthreads();
        if (lane < 16) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += red[wave][k][lane];
            d.gap_partial[((size_t)b * HEAD_BLOCKS + blk) * 16 + lane] = lane < d.gap_c ? s : 0.f;
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int hat_head_fused(const HatHeadDesc* d, void* stream) {
    if (!d || !d->x || !d->w || !d->bias || !d->ln0_g || !d->ln0_b || !d->ln1_g || !d->ln1_b || !d->t || !d->n) return HAT_EINVAL;
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->W < 1 || d->reserved0 != 0) return HAT_EINVAL;
    if ((int64_t)d->H * d->W >= (int64_t)INT32_MAX - 3 * HEAD_BLOCKS * 16) return HAT_EINVAL;   // (pixel indices two tiles ahead stay int32)
    if (d->Kpad < HKS * 32 || d->Kpad % 32 || d->ldn < HC || d->ldn % 8) return HAT_EINVAL;
    if (d->gap_c < 0 || d->gap_c > 16 || d->gap_c % 4 || (d->gap_c > 0) != (d->gap_partial != nullptr)) return HAT_EINVAL;
    if (d->dtype != HAT_F32 && d->dtype != HAT_BF16) return HAT_EINVAL;
    if (d->dtype != HAT_BF16 || d->C != HC) return HAT_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(d->x) & 3) || !aligned16(d->w) || !aligned16(d->bias) || !aligned16(d->ln0_g) || !aligned16(d->ln0_b) ||
        !aligned16(d->ln1_g) || !aligned16(d->ln1_b) || !aligned16(d->f0) || !aligned16(d->t) || !aligned16(d->n) || !aligned16(d->n16) ||
        !aligned16(d->gap_partial))
        return HAT_EINVAL;
    dim3 grid(HEAD_BLOCKS / HEAD_WAVES, d->B), block(HEAD_WAVES * 64);
    HAT_LAUNCH(head_fused_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), *d);
    return hat_check_launch();
}
