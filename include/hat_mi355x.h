/*
 * hat_mi355x.h — C ABI of libhat_mi355x.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * forward pass of the HAT super-resolution network of imjaegyun/super_resolution.
 *
 * The reference implements this path in pure PyTorch (no FFI exists upstream); each entry point
 * below replaces a group of ATen calls inside `HAT.forward`.  File:line references are relative
 * to /root/reference/HAT.  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative HAT_E* code on a bad argument or the
 *     (positive) hipError_t of a failed launch; the Python host turns non-zero into RuntimeError;
 *   - all pointers are DEVICE pointers owned by the caller; nothing is allocated, freed or
 *     synchronised inside; kernels are enqueued on `stream` (a hipStream_t passed as void*);
 *   - activations are channel-last ("tokens": (B, H, W, C) == the reference's (B, N, C) layout,
 *     hat_arch.py:571-575); `dtype` selects the storage/MFMA operand type of T-typed buffers:
 *     HAT_F32 (exact fp32 MFMA, parity path) or HAT_BF16 (bf16 MFMA operands, fp32 accumulate);
 *   - the residual stream, LayerNorm statistics, softmax and all accumulations are fp32.
 */
#ifndef HAT_MI355X_H
#define HAT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever a descriptor layout, a packed-weight layout or the entry-point table changes (2: round 3 — HatConvDesc /
 * HatFfnDesc grew in round 2 without a bump; hat_hab_tail3 and its packing; plan files carry the version) */
#define HAT_ABI_VERSION 2

enum { HAT_F32 = 0, HAT_BF16 = 1 };
enum { HAT_EINVAL = -1, HAT_ELDS = -2, HAT_EUNSUPPORTED = -3 };

/* activation codes */
enum { HAT_ACT_NONE = 0, HAT_ACT_GELU = 1 /* exact erf, nn.GELU() */, HAT_ACT_LRELU = 2 /* slope 0.01 */,
       HAT_ACT_LRELU02 = 3 /* slope 0.2 (ESCReal's to_img head): hat_conv's own kernel only; the resident-weight 3x3 kernel
                              declines it, hat_linear and hat_conv3x3_small return HAT_EUNSUPPORTED */ };
/* conv input modes */
enum { HAT_X_NHWC_T = 0, HAT_X_NHWC_F32 = 1, HAT_X_NCHW_F32_MEAN = 2 };
/* conv output modes */
enum { HAT_O_NHWC_T = 0, HAT_O_NHWC_F32 = 1, HAT_O_PIXSHUF_T = 2, HAT_O_NCHW_F32 = 3,
       HAT_O_FOLD2_NCHW_F32 = 4 /* the folded ending as a conv: ksize 5, Cin 64, x_mode HAT_X_NHWC_T, w / bias packing.pack_upfold's
                                   variants, out (B,3,2H,2W) fp32 = v*out_scale + mean[colour]; hat_conv hands the launch to
                                   hat_upfold_to_planes (below) and takes no residual, activation, colsum or LayerNorm with it.
                                   This is the form a forward plan records the folded ending in. */ };

/*
 * Implicit-GEMM convolution / pointwise linear on channel-last data with a fused epilogue:
 *     out[p, n] = epi( sum_{tap, ci} X[p + tap, ci] * Wp[n, tap * Cin_p + ci] + bias[n] )
 * zero padding ksize/2, stride 1.  Replaces (ksize == 1) nn.Linear / 1x1 nn.Conv2d:
 * hat_arch.py:111,117 (FFN fc1/fc2), :347,350,391 (OCAB q/kv/proj), :309-313 (OCAB MLP),
 * esc_arch.py:144 (ESC aggr); (ksize == 3) hat_arch.py:84,86 (CAB), :544 (RHAG conv), :673,747,
 * 754,757 (head/tail), :598,601 (Upsample convs, with nn.PixelShuffle :599,602 folded into the
 * store); (ksize == 13) esc_arch.py:122-123 (large-kernel conv + dynamic depthwise conv, the
 * latter folded into per-sample weights by hat_esc_weights).
 *
 * Wp is packed [n_slices * nt * 16][Kpad] in T with K index = tap * Cin_p + ci,
 * Cin_p = round_up(Cin, 8), Kpad = round_up(ksize^2 * Cin_p, KC), KC = 64 (bf16) / 32 (f32), x3 when nt == 1;
 * zero padded.  epi: v = acc + bias[n]; v = act(v); v += r1[p, n] (fp32, optional);
 * v += r2scale[n] * r2[p, n] (T, optional); store by out_mode; optional per-tile column sums
 * of v (for the ECA global average pool, hat_arch.py:73).
 */
typedef struct HatConvDesc {
    const void* x;        /* main input */
    const void* x0;       /* optional: channels [0, c_split) are read from x0 (NHWC T, ldx0) */
    const void* w;        /* packed weights (T) */
    const float* bias;    /* [n_slices*nt*16] fp32, zero padded */
    void* out;
    const float* r1;      /* optional fp32 residual, NHWC stride ldr1 (FP16 rows when reserved0 bit 0 is set) */
    const void* r2;       /* optional T residual, NHWC stride ldr2, scaled per channel by r2scale */
    const float* r2scale; /* [B][r2scale_bstride] fp32 */
    float* colsum;        /* optional [B][tiles][n_slices*nt*16] per-tile column sums */
    int32_t B, H, W;
    int32_t Cin, ldx, x_mode;
    int32_t c_split, ldx0;
    int32_t ksize, Kpad;
    int32_t nt, n_slices;
    int64_t w_bstride;    /* elements between per-sample weight sets (0 = shared) */
    int32_t n_store;      /* channels actually stored (multiple of 4 unless out_mode NCHW) */
    int32_t ldo, out_mode, act;
    int32_t ldr1, ldr2, r2scale_bstride;
    int32_t ps_r;         /* pixel-shuffle factor for HAT_O_PIXSHUF_T */
    float in_scale, out_scale;
    float mean[4];        /* HAT_X_NCHW_F32_MEAN: x = (x - mean[c]) * in_scale;  HAT_O_NCHW_F32: v*out_scale + mean[n] */
    int32_t dtype;
    /* hat_linear only (n_slices == 1, n_store == channels): also emit LayerNorm(v) (eps 1e-5) of the finished pixel,
     * i.e. the nn.LayerNorm that consumes this layer's output (hat_arch.py:214 after :236; :306 after :391), as T
     * rows of ld_ln elements.  ln_ones != 0: element [n_store] of every row is 1.0 and the rest up to ld_ln is 0 —
     * the image hat_ffn's m_in expects.  ln_out == NULL: off. */
    int32_t ld_ln, ln_ones;
    const float* ln_g;
    const float* ln_b;
    void* ln_out;
    /* hat_conv with ln_out (n_slices == 1, n_store == 16 nt, NHWC output, ln_ones == 0): the same fused LayerNorm in
     * the conv's epilogue — the norm1 of the next residual group's first block, or HAT.norm, after the group conv
     * (hat_arch.py:556 then :214 / :844) — with what the ESC path of that block needs from it:
     * gap_out (B, hat_conv_tiles, 16) per-tile sums of the first gap_c (<= 16, % 4) LayerNorm channels over the tile's
     * pixels (the partial sums hat_esc_weights reduces), n16_out (B,H,W,16) T a compact copy of LayerNorm channels
     * [0,16).  Both optional (NULL). */
    float* gap_out;
    void* n16_out;
    int32_t gap_c;
    /* The residual stream as FP16 rows (B,H,W,C) instead of fp32 ones: bit 0 = r1 is FP16 rows (8-byte aligned), bit 1 = the
     * HAT_O_NHWC_F32 output is stored as FP16 rows (16-byte aligned, ldo % 8 == 0; round to nearest, clamped to +-65504).
     * Conversion on load is exact.  The fused LayerNorm, its GAP partials and n16_out are computed from the UNROUNDED fp32
     * result, as hat_hab_tail3 does with an FP16 t_out.  Accepted by hat_conv for bf16, nt == 9, one slice, n_store == 144,
     * ksize > 1, no colsum (the group conv of the embed_dim-144 models; r1 == out in place works as with fp32), and by
     * hat_linear for bf16, nt == 9, Cin <= 160, fp32 output with r1 only, one slice, ln_ones == 0 (the OCAB projection,
     * with or without its fused LayerNorm).  HAT_EINVAL elsewhere; 0 = both fp32. */
    int32_t reserved0;
} HatConvDesc;

/* Debug query (not thread safe): how many workgroups of the kernel hat_conv would launch for `d` fit one CU. */
int hat_conv_occupancy(const HatConvDesc* d, int32_t* wgs_per_cu);
/* Number of spatial tiles hat_conv uses for (H, W, Cin, ksize, nt, dtype): the leading dimension of `colsum`. */
int hat_conv_tiles(const HatConvDesc* d, int32_t* tiles_out);
/* The launch plan hat_conv picks for `d`: waves per workgroup, pixel rows per wave, spatial tiles and dynamic
 * LDS bytes.  The kernel instantiation is conv_kernel<T, waves, rows_per_wave, nt> (used to label profiles). */
int hat_conv_plan(const HatConvDesc* d, int32_t* waves, int32_t* rows_per_wave, int32_t* tiles, int64_t* lds_bytes);
int hat_conv(const HatConvDesc* d, void* stream);
/*
 * hat_conv with the FP16-range guard of the residual stream.  A launch that stores FP16 rows (reserved0 bit 1) clamps what lies
 * beyond +-65504 and, by itself, records nothing.  The guarded launch stores the same bytes into every output and also watches
 * the fp32 values it converts, before the clamp, at the pixels it stores (not at the pixels of a ragged tile beyond H or W):
 * if one has a magnitude above 65504, or is an infinity or a NaN, *sat is raised (atomic maximum, as an unsigned integer) to the
 * fp32 bit pattern of its magnitude.  The caller zeroes *sat; a word that is still 0 after the launches of a forward says that
 * no FP16 store of that forward clipped, any other word is the largest offending magnitude (a NaN's pattern above all).
 * sat: device memory, 4-byte aligned.  sat == NULL: hat_conv.  With sat set, a descriptor that stores no FP16 rows (reserved0
 * bit 1 clear) or a misaligned sat returns HAT_EINVAL.  Forward plans record hat_conv, never this entry.
 */
int hat_conv_guarded(const HatConvDesc* d, uint32_t* sat, void* stream);

/*
 * Pointwise linear layer (ksize == 1, channel-last T input, HAT_O_NHWC_T / HAT_O_NHWC_F32 output, same epilogue
 * as hat_conv without column sums) as a weight-stationary, barrier-free streaming GEMM: the layers it serves
 * (hat_arch.py:309-313,347,350,391; esc_arch.py:144) are HBM-bound.  Same descriptor as hat_conv, but `w` is
 * FRAGMENT packed: [n_slices][nt][ceil(Cin/32)][64 lanes][8] with element (lane l, j) =
 * W[slice*nt*16 + t*16 + (l & 15)][32*ks + 8*(l >> 4) + j] (zero beyond Cin / n); Kpad is ignored.
 * Returns HAT_EUNSUPPORTED for (nt, Cin) pairs that are not instantiated: call hat_conv instead.
 */
int hat_linear(const HatConvDesc* d, void* stream);
/*
 * hat_linear with the FP16-range guard: hat_conv_guarded's contract for the launch that stores FP16 rows (reserved0 bit 1: the
 * OCAB projection).  Lanes beyond the last pixel re-store the last pixel and count its values again; nothing else is counted.
 * sat == NULL: hat_linear.  reserved0 bit 1 clear with sat set, or a misaligned sat: HAT_EINVAL.
 */
int hat_linear_guarded(const HatConvDesc* d, uint32_t* sat, void* stream);

/*
 * 3x3 convolution (zero padding 1) whose whole weight slice fits in LDS — the two CAB convolutions
 * (hat_arch.py:84,86) — in the same free-running structure: neighbour pixels are gathered straight from global
 * memory.  Same descriptor as hat_conv (ksize 3, n_slices 1, channel-last T input, no residuals), weights
 * FRAGMENT packed like hat_linear with K index = tap * Cin_p + ci.  Optional colsum is [B][groups][nt*16]
 * (one row per workgroup), groups from hat_conv3x3_small_groups().  HAT_EUNSUPPORTED: use hat_conv.
 */
int hat_conv3x3_small_groups(const HatConvDesc* d, int32_t* groups_out);
int hat_conv3x3_small(const HatConvDesc* d, void* stream);

/*
 * CAB expand conv + ECA folded into the ESC aggregation (hat_arch.py:84-90, 66-78, 233-236 with esc_arch.py:123) for
 * models whose CAB squeeze width is <= 8 channels (HAT-S: 6).  The reference computes
 *     c2 = conv3x3(c1) + b2;  e = sigmoid(conv1d_k(mean_pixels(c2)));  x = t + aggr(y) + conv_scale * e * c2.
 * mean_pixels(c2) is linear in c1, so it follows from the column sums of c1 and its border rows / columns
 * (zero padding: tap (dy,dx) misses one border row and/or column), BEFORE c2 exists:
 *   hat_cab_fold:  scale = conv_scale * e,  wf = fragment-packed (scale * W2) with K = tap*8 + ci,
 *                  bias_out = bias_in + scale * b2            (tiny per-sample kernel)
 *   hat_aggr_cab:  out = r1 + W_aggr . x + wf . im2col3x3(c1) + bias_out   — c2 never exists in memory.
 */
typedef struct HatCabFoldDesc {
    const void* c1;          /* (B,H,W,ld1) T: GELU(conv3x3(n)), `mid` channels, pad channels zero, ld1 == 8 */
    const float* c1_colsum;  /* [B][tiles][ldcs]: per-tile column sums of c1 as hat_conv's colsum emits them */
    const float* w2;         /* [C][mid][3][3] fp32 */
    const float* b2;         /* [C] */
    const float* wk;         /* ECA conv1d weights [k] */
    const float* bias_in;    /* [C]: the aggregation bias */
    float* scale;            /* out [B][ld_scale] */
    void* wf;                /* out [B][nt][3][64][8] T, nt = ceil(C/16) */
    float* bias_out;         /* out [B][nt*16] */
    float* tmp;              /* scratch [B][32][ldcs] */
    int32_t B, H, W, C, mid, ld1, tiles, ldcs, k, ld_scale, dtype;
    float conv_scale;
    /* optional [B][72] fp32: the sums this kernel otherwise takes from c1 / c1_colsum, supplied by the caller — a frame that is
     * sharded into row bands adds up its bands' hat_rect_sum results: [0,8) sums of c1's channels over the whole
     * frame, [8,40) over its first row, last row, first column, last column, [40,72) its four corner pixels (top-left,
     * top-right, bottom-left, bottom-right).  H, W are then the FULL frame's; c1, c1_colsum, tmp are not read. */
    const float* stats;
    /* optional: W2 once more, in wf's own order, fp32 [nt][3][64][8] with element (t, ks, lane, j) = W2[16 t + (lane & 15)][ci = j]
     * [tap = 4 ks + (lane >> 4)] (zero where co >= C, tap >= 9 or ci >= mid).  The kernel then reads the weights it scales with
     * unit stride (it is ONE workgroup on the critical chain of a block: the gather out of the [C][mid][3][3] layout was half
     * of its time).  NULL: gather from w2. */
    const float* w2f;
} HatCabFoldDesc;
int hat_cab_fold(const HatCabFoldDesc* d, void* stream);

typedef struct HatAggrCabDesc {
    HatConvDesc lin;         /* the aggregation as for hat_linear: x (+x0 / c_split), w (fragment packed, nt = 9, Cin = 144),
                                out (fp32, HAT_O_NHWC_F32), r1 (fp32); bias, r2*, ln_* are ignored */
    const void* c1;          /* (B,H,W,8) T */
    const void* wf;          /* hat_cab_fold's wf */
    const float* bias_b;     /* hat_cab_fold's bias_out, [B][nt*16] */
} HatAggrCabDesc;
int hat_aggr_cab(const HatAggrCabDesc* d, void* stream);

/*
 * LayerNorm over the channel dimension (eps 1e-5, affine), fp32 in -> T or fp32 out
 * (nn.LayerNorm at hat_arch.py:209,214,291,306,743 and PatchEmbed.norm :573-574).
 * Optionally emits per-block partial sums of the first `gap_c` (<= 32, % 4) output channels
 * (the AdaptiveAvgPool2d(1) feeding the ESC dynamic kernel, esc_arch.py:96,121):
 * gap_partial[b][blk][gs], blk < hat_layernorm_blocks(), gs = 16 floats per block, 32 when gap_c > 16.
 */
int hat_layernorm_blocks(void);
int hat_layernorm(const float* x, void* y, const float* gamma, const float* beta, float* gap_partial,
                  int32_t B, int64_t npix, int32_t C, int32_t ldy, int32_t out_f32, int32_t gap_c,
                  int32_t dtype, void* stream);

/*
 * The head of the network in ONE launch (embed_dim 144, in_chans 3, bf16; hat_arch.py:836-837, :849-850 and the first
 * block's norm1 :209): what hat_conv (conv_first, HAT_X_NCHW_F32_MEAN -> HAT_O_NHWC_F32), hat_layernorm (patch-embed norm,
 * fp32 -> fp32) and hat_layernorm (norm1, fp32 -> bf16 rows with GAP partials) compute in three, bit for bit:
 *     f0 = conv3x3((x - mean) * in_scale) + bias;  t = LayerNorm(f0; ln0);  n = bf16(LayerNorm(t; ln1))
 * The conv runs on hat_conv's packed weights with hat_conv's k order (k = tap * 8 + ci, three 32-deep MFMA steps, the bias
 * added in fp32 behind them), both LayerNorms on the accumulators with hat_layernorm's formula and summation tree, so
 * every output equals the three-launch result.  A wave owns block `blk` of hat_layernorm's pixel partition (16 consecutive
 * pixels every hat_layernorm_blocks() * 16), which makes gap_partial hat_layernorm's, block for block.
 *   x (B,3,H,W) fp32 planes;  w [144][Kpad] bf16, bias [144] fp32: hat_conv's packing of conv_first (nt = 9, one slice);
 *   f0, t (B,H*W,144) fp32 (f0 NULL: not stored);  n (B,H*W,ldn) bf16, ldn >= 144, % 8;  n16 (B,H*W,16) bf16 or NULL: a
 *   compact copy of n's first 16 channels;  gap_partial (B, hat_layernorm_blocks(), 16) fp32, sums of the STORED n over the
 *   first gap_c in {0, 4, 8, 12, 16} channels (NULL with gap_c = 0).
 * HAT_EUNSUPPORTED: dtype != HAT_BF16 or C != 144.  HAT_EINVAL: anything else out of range, H * W >= 2^31 - 2^15, a pointer
 * that is not 16-byte aligned (x: 4).
 */
typedef struct HatHeadDesc {
    const float* x;
    const void* w;
    const float* bias;
    const float* ln0_g;      /* patch-embed norm, [144] each */
    const float* ln0_b;
    const float* ln1_g;      /* the first block's norm1 */
    const float* ln1_b;
    float* f0;
    float* t;
    void* n;
    void* n16;
    float* gap_partial;
    int32_t B, H, W, C;
    int32_t Kpad;            /* row stride of w in elements: >= 96, % 32 */
    int32_t ldn, gap_c, dtype;
    float in_scale;
    float mean[4];           /* per input channel; [3] unused */
    int32_t reserved0;       /* 0 */
} HatHeadDesc;
int hat_head_fused(const HatHeadDesc* d, void* stream);

/*
 * out[b][i] = a[b][i] + c[b * c_bstride + i], i < n (fp32, n % 4 == 0; out may alias a).  The plain adds of the
 * reference that no producing kernel can absorb: the absolute position embedding (hat_arch.py:837-838,
 * c_bstride = 0: broadcast over the batch) and the residuals around nn.Identity when
 * resi_connection == 'identity' (:545-546 with :556, :748 with :854).
 */
int hat_add_f32(const float* a, const float* c, float* out, int32_t B, int64_t n, int64_t c_bstride, void* stream);

/*
 * ESC per-sample conv weights (esc_arch.py:95-100,121-123): p = mean(gap partials);
 * dk = W2 * gelu(W1 * p + b1) + b2 (pdim*9 values); Wp[b][co][tap*Cin_p + ci] =
 * T( plk_packed[co][tap*Cin_p+ci] + (co == ci && tap in central 3x3 ? dk[co*9 + ..] : 0) ).
 * pdim <= 32 (% 4): the GAP partial blocks are 16 floats (32 for pdim > 16, hat_layernorm's layout for gap_c = pdim) and
 * plk_packed / w_out hold 16 rows per sample (32 for pdim > 16: two 16-row slices for hat_conv with nt = 1).
 */
int hat_esc_weights(const float* gap_partial, int32_t nblk, int64_t npix, const float* w1, const float* b1,
                    const float* w2, const float* b2, const float* plk_packed, void* w_out, int32_t B,
                    int32_t pdim, int32_t ksize, int32_t Kpad, int32_t dtype, void* stream);

/*
 * The ESC large-kernel conv as a dedicated kernel (esc_arch.py:121-123), bf16, pdim 16, 13x13: y16 = conv2d(x[..., :16], Wp[b])
 * with zero padding 6, no bias.  x: (B,H,W,ldx) T (the first 16 channels are used); wp: hat_esc_weights' output
 * [B][16][Kpad] (K = tap * 16 + ci, tap = ty * 13 + tx); y16: (B,H,W,16) T.  All weights and the haloed tile stay in LDS.
 * HAT_EUNSUPPORTED for other dtypes: use hat_conv (ksize 13).
 */
int hat_esc_conv13(const void* x, int32_t ldx, const void* wp, int32_t Kpad, void* y16, int32_t B, int32_t H, int32_t W,
                   int32_t dtype, void* stream);

/*
 * ECA channel attention scale (hat_arch.py:73-77) times conv_scale (:236):
 * scale[b][c] = conv_scale * sigmoid( conv1d_k(mean_pixels(c2))[c] ), from hat_conv's colsum.
 * `tmp` is fp32 scratch of B*32*ldc floats.
 */
int hat_eca_scale(const float* colsum, int32_t tiles, int32_t ldc, int64_t npix, const float* wk, int32_t k,
                  float conv_scale, float* tmp, float* scale, int32_t B, int32_t C, void* stream);

/*
 * Depthwise 3x3 (+bias, zero pad) on 2*hid channels, chunk(2), a * SiLU(g)   (hat_arch.py:112-116).
 * u: (B,H,W,ldu) T with 2*hid channels; wdw packed [9][2*hid] fp32; out (B,H,W,ldo) T with hid channels.
 */
int hat_dwconv_gate(const void* u, const float* wdw, const float* bdw, void* out, int32_t B, int32_t H,
                    int32_t W, int32_t hid, int32_t ldu, int32_t ldo, int32_t dtype, void* stream);

/*
 * The OCAB's MLP with its residual in one launch (hat_arch.py:309-313, :391): out = r1 + fc2(GELU(fc1(x))), exact-erf GELU
 * (the bf16 path's approximation of hat_linear), for embed_dim 144, hidden 288, bf16 (HAT_EUNSUPPORTED otherwise: run the two
 * hat_linear launches).  The hidden tensor stays in registers.
 *   x    (B,H,W,ldx) T: LayerNorm2 output;  r1 (B,H,W,ldr1) fp32: the residual stream;
 *   out  (B,H,W,ldo): fp32 when out_f32 == 1 (may alias r1), else T rows (16-byte aligned, ldo % 8 == 0);
 *   out_f32 == 2: T rows out and r1 is FP16 rows (8-byte aligned; the 16-bit residual stream, converted exactly); 3 is HAT_EINVAL;
 *   w1f  fc1 as MFMA A fragments [18 n-tiles][4 k-steps][64 lanes][8] bf16 (rows = hidden unit 16 nt + (lane & 15), k = 32 ks +
 *        8 (lane >> 4) + j), followed by the 16-deep tail [18][64 lanes][4] (k = 128 + 4 (lane >> 4) + j);  b1 [288] fp32;
 *   w2f  fc2 as A fragments [9 n-tiles][9 k-steps][64 lanes][8] bf16, rows = output channel, k-slot (g = lane >> 4, j) of k-step kk =
 *        hidden unit 32 kk + 4 g + j (j < 4) or 32 kk + 16 + 4 g + j - 4 (j >= 4);  b2 [144] fp32.
 */
typedef struct HatMlpDesc {
    const void* x;
    const void* w1f;
    const float* b1;
    const void* w2f;
    const float* b2;
    const float* r1;
    void* out;
    int32_t B, H, W, C, hidden;
    int32_t ldx, ldr1, ldo;
    int32_t out_f32, dtype;
} HatMlpDesc;
int hat_ocab_mlp(const HatMlpDesc* d, void* stream);
/*
 * The OCAB's q and kv projections (hat_arch.py:347, :350) in one launch for embed_dim 144, bf16: out rows of 432 channels
 * [q | k | v] (T, 16-byte aligned, ldo % 8 == 0) = W x + b.  Uses HatMlpDesc: x, ldx as above; w1f = the stacked weight
 * [q_proj * head_dim^-0.5 ; kv_proj] (432 x 144) in hat_ocab_mlp's fc1 fragment layout ([27][4][64][8] + [27][64][4]); b1 [432]
 * (q part scaled likewise); hidden = 432; w2f, b2, r1, ldr1, out_f32 unused.  hat_ocab_attention then takes q = out,
 * kv = out + 144 elements, ldq = ldkv = ldo.
 */
int hat_ocab_qkv(const HatMlpDesc* d, void* stream);

/*
 * HATX's OCAB options (hatx_arch.py:421-449), for the key windows the generic attention kernel is built for (wse = 24, 12 and
 * the odd 25, 13):
 *   hat_ocab_keybias      kb[b][window][key] (fp32, rows of round_up(wse*wse, 16) floats per window: whole key tiles) = tanh(sal at the key's pixel) for a kept key — 0
 *                         without a focus head (sal == NULL: the score is then ||k||_2 over the C key channels of kv) —
 *                         and -inf for a pruned one; kept = the k_keep keys of a window with the largest score, ties by
 *                         the lower key index (the reference leaves tie order to torch.topk); zero-padded keys outside
 *                         the image score tanh(0) = 0 / norm 0.  sal: (B,H,W,ldsal) T, channel 0 = the saliency map.
 *   hat_ocab_attention_kb hat_ocab_attention with `kb` applied before the relative-position bias: logit + kb, or -1e4 in
 *                         place of the logit where kb = -inf; `pad` = ceil((wse - ws) / 2), HATX's unfold padding.
 * ldsal < 0 (dtype HAT_BF16 only): `sal` is an FP32 map of row stride -ldsal — the saliency head's last conv writes its fp32
 * accumulators (HAT_O_NHWC_F32) so that the keys are ranked on unrounded scores; kv stays bf16.
 * hat_ocab_keybias writes 0 into the dead tail [wse*wse, round_up(wse*wse, 16)) of a row; hat_ocab_attention_kb ignores what
 * is there.  A key's rank is the number of keys that compare greater (or equal, at a lower index), so a NaN score — a NaN in
 * the saliency map or in k — compares with nothing, ranks 0 and is kept (with kb = NaN under a focus head), and more than k_keep keys of that window
 * survive: the maps must be finite (the engine's are; nothing here checks).
 */
int hat_ocab_keybias(const void* sal, int32_t ldsal, const void* kv, int32_t ldkv, float* kb, int32_t B, int32_t H, int32_t W,
                     int32_t C, int32_t ws, int32_t wse, int32_t pad, int32_t k_keep, int32_t dtype, void* stream);
int hat_ocab_attention_kb(const void* q, const void* kv, const float* bias_rot, const float* kb, void* out, int32_t B, int32_t H,
                          int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t pad, int32_t ldq, int32_t ldkv,
                          int32_t ldo, int32_t dtype, void* stream);

/*
 * Spatial-gate step of HATX's SGFN (hatx_arch.py:165-177) between its fc1 and fc2: depthwise 3x3 (+bias, zero pad) on the
 * FIRST `half` channels of u, gated by SiLU of the second half, which is also passed on:
 *     out[..., :half] = dw3x3(u[..., :half]) * SiLU(u[..., half:]),   out[..., half:] = u[..., half:].
 * u: (B,H,W,ldu) T with 2*half channels; wdw packed [9][half] fp32, bdw [half]; out (B,H,W,ldo) T, must not alias u.
 */
int hat_sgfn_gate(const void* u, const float* wdw, const float* bdw, void* out, int32_t B, int32_t H, int32_t W,
                  int32_t half, int32_t ldu, int32_t ldo, int32_t dtype, void* stream);

/*
 * Overlapping cross-attention core (hat_arch.py:353-388): per 'ws x ws' query window and head,
 * softmax(q k^T + RPB) v over the 'wse x wse' key window (stride ws, zero padded, NOT masked).
 * q: (B,H,W,ldq) T (already multiplied by head_dim^-0.5), kv: (B,H,W,ldkv) T with k at channel 0
 * and v at channel C; bias_rot: [heads][(ws+wse-1)^2] fp32, the relative-position-bias table
 * rotated so that index (kh-qh+ws-1)*(ws+wse-1) + (kw-qw+ws-1) is non-negative (the reference's
 * negative-index wraparound, hat_arch.py:378, is applied when the table is packed).
 * out: (B,H,W,ldo) T in window_reverse order (:387-388).
 * Key windows: wse = 24 and 12 (window 16 / 8, overlap 0.5; padding (wse - ws) / 2 on every side) and the odd 25 and 13
 * (HATX: overlap 0.6 / 0.7, padding ceil((wse - ws) / 2), hatx_arch.py:303-305); HAT_EUNSUPPORTED for others.  When
 * K and V of one key window do not fit the LDS (fp32, wse 25, head_dim 30) a 16 x 16 window streams its keys through the LDS
 * in chunks (same arithmetic, same key order); HAT_ELDS for other window sizes in that case.
 * Nothing beyond element alignment is required of q, kv and out: the tuned bf16 kernels (ws 16, wse 24, head_dim 24 / 30) are taken
 * only when strides AND pointers allow their 16- / 8-byte (head_dim 24) or 4-byte (head_dim 30) accesses, the generic kernel otherwise.
 */
int hat_ocab_attention(const void* q, const void* kv, const float* bias_rot, void* out, int32_t B, int32_t H,
                       int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t ldq,
                       int32_t ldkv, int32_t ldo, int32_t dtype, void* stream);
/*
 * hat_ocab_attention for the tuned kernel of the embed_dim-144 models (bf16, 16 x 16 windows, 24 x 24 key windows, head_dim 24;
 * HAT_EUNSUPPORTED otherwise), with q ALREADY multiplied by head_dim^-1/2 * log2(e) — the caller folds the factor into the q
 * projection's weights before they are rounded, so the scores are in log2 units at no extra rounding.  The kernel then carries
 * the softmax's offset in a spare k-slot of the QK^T MFMA (K rows hold 1.0, the query fragment -offset): p = exp2(score) with no
 * per-score FMA and no rescale of O.  The offset is the row maximum of the first 96-key chunk; the rest of the key window runs
 * without range checks, and a query tile whose softmax denominator comes out non-finite or above 1e30 (a later score more than
 * ~2^100 above the first chunk's maximum) is computed again with a check and a re-centring step per chunk.  Same result as
 * hat_ocab_attention up to rounding (hat_arch.py:375-384).
 */
int hat_ocab_attention_log2(const void* q, const void* kv, const float* bias_rot, void* out, int32_t B, int32_t H, int32_t W,
                            int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t ldq, int32_t ldkv, int32_t ldo,
                            int32_t dtype, void* stream);

/*
 * CAB squeeze conv: GELU_erf(conv3x3(x, C -> mid <= 8 channels, zero pad) + bias)   (hat_arch.py:84-85, cab.0 + GELU)
 * for bf16 rows without LDS operand traffic: a wave sweeps a strip of 14 output columns (16 loaded ones: a halo column on each
 * side) top to bottom, every input row's activations come straight from global memory ONCE (the fragments of the two
 * horizontally shifted taps are lane shifts of the loaded one), the weights stay in registers, and the three taps of a
 * kernel column are routed to three rolling output-row accumulators by the choice of MFMA C operand (csrc/hat_cabsq.hip).
 * x: (B,H,W,ldx) bf16, 128 < C <= 160, C % 8 == 0; W % 16 == 0.
 * wpk: 6 tiles x 5 k-steps of MFMA A fragments [tile][kstep][64 lanes][8] bf16, tile = 2*kx + j:
 *      j = 0: rows 0-7 = w[ch][.][ky=0][kx], rows 8-15 = w[ch][.][ky=1][kx];  j = 1: rows 0-7 = w[ch][.][ky=2][kx], rest 0
 *      (fragment element [lane][e] = row lane%16, input channel 32*kstep + 8*(lane/16) + e; channels >= C are zero).
 * bias: 8 floats (zeros past mid).  out: (B,H,W,8) bf16, channels >= mid are exact zeros.
 * colsum (optional): [B][units][16] fp32 per-wave-unit channel sums of the stored values (what hat_cab_fold consumes as
 * c1_colsum with tiles = units, ldcs = 16); units from hat_cab_squeeze_units.  dtype must be HAT_BF16 (the fp32 parity
 * path uses hat_conv).
 */
int hat_cab_squeeze_units(int32_t H, int32_t W, int32_t* rows_per_band, int32_t* units);
int hat_cab_squeeze(const void* x, const void* wpk, const float* bias, void* out, float* colsum, int32_t B, int32_t H,
                    int32_t W, int32_t C, int32_t ldx, int32_t dtype, void* stream);

/*
 * conv_last (hat_arch.py:757, 856-858): out = (conv3x3(x, 64 -> n_out <= 8) + bias) * out_scale + mean[ch], written as
 * (B, n_out, H, W) fp32 planes — the same row-sweep kernel as hat_cab_squeeze with two k-steps (num_feat = 64,
 * hat_arch.py:656).  x: (B,H,W,ldx) bf16; wpk: 6 tiles x 2 k-steps of A fragments in hat_cab_squeeze's tile order;
 * bias: 8 floats; mean4: 4 floats (the RGB mean, or zeros); W % 16 == 0; dtype must be HAT_BF16.
 */
int hat_conv3x3_to_planes(const void* x, const void* wpk, const float* bias, float* out, int32_t B, int32_t H, int32_t W,
                          int32_t C, int32_t ldx, int32_t n_out, float out_scale, const float* mean4, int32_t dtype,
                          void* stream);

/*
 * The 8-bit frame boundary: interleaved uint8 frames in, interleaved uint8 frames out, with the reference's conversions
 * (basicsr utils/img_util.py:9-35, :131 in; hat/models/hat_model.py:16-26 pad, :110-112 crop; img_util.py:66-91 out).
 *
 * hat_u8_to_planes   src: (B,h,w,3) uint8, rows src_pitch bytes apart (>= 3 w), samples src_bstride bytes apart (ignored for
 *                    B == 1) -> dst: (B,3,Hp,Wp) fp32 planes, dst[b][c][y][x] = float(src[b][y'][x'][bgr ? 2 - c : c]) / 255.0f
 *                    exactly (a 256-entry table of correctly rounded quotients), y' = y for y < h else 2 (h - 1) - y and
 *                    likewise x': rows and columns past the frame are its reflection without the edge (F.pad 'reflect'
 *                    on the bottom and the right).  Hp >= h, Wp >= w; Hp - h >= h or Wp - w >= w (no row / column to
 *                    reflect) is HAT_EINVAL.
 * hat_planes_to_u8   src: (B,3,Hs,Ws) fp32 planes -> dst: (B,h_out,w_out,3) uint8 with dst_pitch >= 3 w_out bytes per row
 *                    and dst_bstride bytes per sample: the top-left h_out x w_out pixels (h_out <= Hs, w_out <= Ws),
 *                    each value clamped to [0, 1], multiplied by 255 in fp32, rounded half to even; plane c goes to
 *                    byte (bgr ? 2 - c : c) of its pixel.  The general output path: any width, any engine dtype.
 * hat_conv3x3_to_u8  conv_last with that conversion as its epilogue: hat_conv3x3_to_planes' kernel, arguments and fp32
 *                    value (conv3x3(x, 64 -> 3) + bias) * out_scale + mean[ch], stored as hat_planes_to_u8 stores it
 *                    (rows >= h_out and columns >= w_out are skipped; h_out <= H, w_out <= W), so the fp32 image is never
 *                    written.  Bit-identical to hat_planes_to_u8 of hat_conv3x3_to_planes.  x: (B,H,W,ldx) bf16,
 *                    W % 16 == 0, C == 64, wpk / bias packed for n_out = 3; dtype must be HAT_BF16.
 * All three check their arguments before they touch the device; none allocates or synchronises.
 */
int hat_u8_to_planes(const uint8_t* src, int64_t src_pitch, int64_t src_bstride, float* dst, int32_t B, int32_t h, int32_t w,
                     int32_t Hp, int32_t Wp, int32_t bgr, void* stream);
int hat_planes_to_u8(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride,
                     int32_t h_out, int32_t w_out, int32_t bgr, void* stream);
int hat_conv3x3_to_u8(const void* x, const void* wpk, const float* bias, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride,
                      int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t h_out, int32_t w_out, float out_scale,
                      const float* mean4, int32_t bgr, int32_t dtype, void* stream);

/*
 * The 4:2:0 frame boundary: YCbCr frames as decoders and encoders exchange them (NV12, NV21, I420) in and out; first with
 * 8-bit samples.  The definition, operation by operation, is super_resolution_amd/yuv.py; the results equal it bit for bit
 * (every product and sum is rounded to fp32 on its own: no fused multiply-add).  A frame block is
 *     y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride
 * — the Y plane (h rows of w bytes, rows y_pitch >= w bytes apart, samples y_bstride bytes apart) and the (h/2, w/2) Cb and
 * Cr samples behind two pointers, rows c_pitch bytes apart, samples of a row c_step bytes apart, samples of the batch
 * c_bstride apart: c_step = 1 for planar chroma (I420), c_step = 2 for interleaved chroma (NV12: cr = cb + 1; NV21: cb = cr +
 * 1), c_pitch >= c_step * w / 2.  The b-strides are ignored for B == 1.  h and w must be even.
 * to_rgb12 / from_rgb12: HOST pointers to 12 floats, a row-major 3 x 4 matrix passed to the kernel by value
 * (super_resolution_amd.yuv.csc(matrix, full_range) makes the pairs for BT.601 / BT.709, limited / full range):
 *     to_rgb    rows R, G, B; columns Y, Cb - 128, Cr - 128, offset   (byte units in, [0, 1] out; the luma offset is part of
 *               the offset column, which is added last)
 *     from_rgb  rows Y, Cb, Cr; columns R, G, B, offset               ([0, 1] in, byte units out)
 *
 * hat_yuv420_to_planes   -> dst: (B,3,Hp,Wp) fp32 RGB planes.  Pixel (y, x) reads source pixel (y', x') by hat_u8_to_planes'
 *                    reflection rule and the chroma sample (y' >> 1, x' >> 1) (nearest: a chroma sample covers its 2 x 2
 *                    block); dst = min(max(((m0 Y + m1 (Cb - 128)) + m2 (Cr - 128)) + m3, 0), 1) per row of to_rgb.
 *                    Refuses what hat_u8_to_planes refuses, odd h or w, short pitches and c_step outside {1, 2}.
 * hat_planes_to_yuv420   src: (B,3,Hs,Ws) fp32 planes -> the top-left h_out x w_out pixels (even, <= Hs, Ws) as a frame
 *                    block.  r, g, b are clamped to [0, 1]; Y = ((k00 r + k01 g) + k02 b) + k03 per pixel; cb = (k10 r + k11
 *                    g) + k12 b per pixel and Cb = ((cb00 + cb01) + (cb10 + cb11)) * 0.25 + k13 per 2 x 2 block (box), Cr
 *                    likewise; a byte is the value clamped to [0, 255] and rounded half to even.  The general output
 *                    path: any width, any engine dtype.
 * hat_conv3x3_to_yuv420  conv_last with that conversion as its epilogue: hat_conv3x3_to_u8's arguments with the destination
 *                    replaced by a frame block, the same kernel and fp32 value; neither the fp32 image nor an RGB byte
 *                    image is written.  Bit-identical to hat_planes_to_yuv420 of hat_conv3x3_to_planes.  Its row bands
 *                    are an even number of rows high (a 2 x 2 block never straddles two bands).
 * Centre-sited chroma (JPEG, MPEG-1, Y4M C420jpeg) is what nearest-up / box-down means, and it is what these entries compute;
 * left- and top-left-sited chroma (MPEG-2, H.264, HEVC, AV1; BT.2020) is "Chroma siting" below.  All three check their
 * arguments before they touch the device; none allocates or synchronises.
 */
int hat_yuv420_to_planes(const uint8_t* y, int64_t y_pitch, int64_t y_bstride, const uint8_t* cb, const uint8_t* cr, int64_t c_pitch,
                         int32_t c_step, int64_t c_bstride, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp,
                         const float* to_rgb12, void* stream);
int hat_planes_to_yuv420(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint8_t* y, int64_t y_pitch, int64_t y_bstride,
                         uint8_t* cb, uint8_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t h_out, int32_t w_out,
                         const float* from_rgb12, void* stream);
int hat_conv3x3_to_yuv420(const void* x, const void* wpk, const float* bias, uint8_t* y, int64_t y_pitch, int64_t y_bstride, uint8_t* cb,
                          uint8_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t B, int32_t H, int32_t W, int32_t C,
                          int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, const float* mean4, const float* from_rgb12,
                          int32_t dtype, void* stream);

/*
 * The same boundary for 10-, 12- and 16-bit video (HEVC Main10, AV1, VP9 profile 2): a sample is a little-endian 16-bit word
 * that holds an n-bit code, n = depth in {10, 12, 16}.  msb = 1: MSB-aligned words (P010 / P012 / P016, what VCN, VA-API and
 * D3D surfaces hold): code = word >> (16 - n), the low bits are ignored, and word = code << (16 - n) on output.  msb = 0:
 * LSB-aligned words (yuv420p10le / p12le, Y4M C420p10 / C420p12): code = min(word, 2^n - 1) — a word above the range saturates —
 * and word = code.  At n = 16 the two are the same.  With k = n - 8 the input is s = float(code) * 2^-k (exact) and then the
 * byte expression above on s, Cb' = s_cb - 128, Cr' = s_cr - 128; the output value v (byte units, computed exactly as above)
 * becomes code = rint(min(max(v * 2^k, 0), 2^n - 1)), half to even.  The matrices are in BYTE units at every depth
 * (super_resolution_amd.yuv.csc(matrix, full_range, depth); limited-range matrices do not depend on the depth).  No
 * transfer function is applied: the network sees the source's own transfer (gamma, PQ, HLG).
 * The three entries take the 8-bit entries' argument lists with uint16_t blocks, then depth and msb.  Pitches, strides and
 * c_step stay in BYTES (decoder surfaces report bytes) and must be even; c_step is 2 (planar) or 4 (interleaved); the pointers
 * are 2-byte aligned.  They refuse all that the 8-bit entries refuse, odd pitches / strides / pointers, a depth outside {10,
 * 12, 16} and an msb outside {0, 1}, before they touch the device; none allocates or synchronises.  4:2:2, 4:4:4, other
 * chroma filters and tone mapping are out of scope.
 */
int hat_yuv420p16_to_planes(const uint16_t* y, int64_t y_pitch, int64_t y_bstride, const uint16_t* cb, const uint16_t* cr, int64_t c_pitch,
                            int32_t c_step, int64_t c_bstride, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp,
                            const float* to_rgb12, int32_t depth, int32_t msb, void* stream);
int hat_planes_to_yuv420p16(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint16_t* y, int64_t y_pitch, int64_t y_bstride,
                            uint16_t* cb, uint16_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t h_out, int32_t w_out,
                            const float* from_rgb12, int32_t depth, int32_t msb, void* stream);
int hat_conv3x3_to_yuv420p16(const void* x, const void* wpk, const float* bias, uint16_t* y, int64_t y_pitch, int64_t y_bstride, uint16_t* cb,
                             uint16_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, const float* mean4, const float* from_rgb12,
                             int32_t dtype, int32_t depth, int32_t msb, void* stream);

/*
 * The same boundary at any chroma subsampling: 4:2:0, 4:2:2, 4:4:4 and grey, 8 to 16 bits, described ONCE per surface instead
 * of by a growing argument list.  A HatYuvSurface is the frame block of the 4:2:0 entries plus what they imply:
 *     y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride     as above, BYTES everywhere
 *     sub_x, sub_y   log2 of the chroma subsampling: (1,1) 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4; the chroma planes are
 *                    (h >> sub_y, w >> sub_x); w is even where sub_x = 1 and h where sub_y = 1, every other size >= 1 is a frame
 *     depth, msb     8 (bytes; msb is 0 or 1 and not used) or 10 / 12 / 16 (16-bit words, msb as in the deep entries; pointers,
 *                    pitches and strides even); c_step is bps (planar: I422, I444) or 2 bps (interleaved: NV16 / P210, NV24 / P410)
 *     cb = cr = NULL a grey surface (Y only): sub_x, sub_y and the chroma fields are not read.  In: Cb' = Cr' = 0 exactly and the
 *                    same expression follows.  Out: only Y is stored.  ONE of the two NULL is an error.
 * The definition is super_resolution_amd/yuv.py (yuv_to_planes / planes_to_yuv), and the results equal it bit for bit.  In:
 * the chroma sample of source pixel (y', x') is (y' >> sub_y, x' >> sub_x) (nearest).  Out: Y and the per-pixel cb / cr terms as
 * in hat_planes_to_yuv420, then 4:2:0 as there; 4:2:2: C = (c0 + c1) * 0.5 + k[c][3] (left + right); 4:4:4: C = c + k[c][3].
 * hat_yuv_to_planes / hat_planes_to_yuv / hat_conv3x3_to_yuv are hat_yuv420_to_planes / hat_planes_to_yuv420 /
 * hat_conv3x3_to_yuv420 (and their p16 forms) with a surface for the block; for a (1,1) surface they launch the same kernels
 * and write the same samples.  hat_conv3x3_to_yuv takes hat_conv3x3_to_yuv420's conv arguments.  A bad surface (odd w with
 * sub_x = 1, one chroma pointer NULL, c_step not bps / 2 bps, an odd pitch for words, overlapping batch strides, sub_y >
 * sub_x ...) returns HAT_EINVAL before anything touches the device; none allocates or synchronises.  Packed 4:2:2 (YUY2 / UYVY /
 * Y210 / v210) has a descriptor of its own: "Packed 4:2:2" below.  4:1:1, 4:4:0, alpha planes and tone mapping are out of
 * scope.  These entries are centre-sited chroma; see "Chroma siting" below for the rest.
 */
typedef struct {
    void* y; int64_t y_pitch, y_bstride; void* cb; void* cr; int64_t c_pitch; int32_t c_step; int64_t c_bstride;
    int32_t sub_x, sub_y, depth, msb;
} HatYuvSurface;
int hat_yuv_to_planes(const HatYuvSurface* src, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp, const float* to_rgb12,
                      void* stream);
int hat_planes_to_yuv(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatYuvSurface* dst, int32_t h_out, int32_t w_out,
                      const float* from_rgb12, void* stream);
int hat_conv3x3_to_yuv(const void* x, const void* wpk, const float* bias, const HatYuvSurface* dst, int32_t B, int32_t H, int32_t W, int32_t C,
                       int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, const float* mean4, const float* from_rgb12,
                       int32_t dtype, void* stream);

/*
 * The folded ending of the network: the last Upsample conv (3x3, 64 -> 256), its PixelShuffle(2) and conv_last (3x3, 64 -> 3) as one
 * 5x5 conv on x, the (B,H,W,ldx) bf16 input of that Upsample conv; the results are 2H x 2W.  No 64-channel map at output size is
 * written or read.  wpk / bias: packing.pack_upfold's twelve weight variants, bf16 [12][50][64][8] fragments and fp32 [12][16]
 * (variant 3 rs + cs: which neighbour rows / columns of a pixel lie outside the image; a shift of the shuffled map that falls
 * outside is absent as a whole, so every pixel, corners included, is the composition's in exact arithmetic), both 16-byte aligned.
 * The fp32 value of every entry is (conv + bias) * out_scale + mean of the colour, by one expression:
 *   hat_upfold_to_planes  (B,3,2H,2W) fp32 planes, what hat_conv3x3_to_planes writes after hat_conv's PixelShuffle stage;
 *   hat_upfold_to_u8      the bytes hat_planes_to_u8 makes of those planes (top-left h_out x w_out, h_out <= 2H, w_out <= 2W);
 *   hat_upfold_to_yuv     the samples hat_planes_to_yuv makes of them (centre-sited chroma; any subsampling, depth, grey).
 * W % 16 == 0, W >= 16, H >= 1, ldx >= 64, ldx % 8 == 0; dtype must be HAT_BF16 (HAT_EUNSUPPORTED otherwise).  Arguments are
 * checked before anything touches the device; none allocates or synchronises.  hat_conv with out_mode HAT_O_FOLD2_NCHW_F32 is
 * hat_upfold_to_planes behind a HatConvDesc: the engine launches the planes form that way, so a forward plan records it as a
 * hat_conv call (the plan's function table is unchanged and plans written before still load), and hat_plan_forward_u8 / _yuv*
 * replay such a last call as hat_upfold_to_u8 / hat_upfold_to_yuv.
 */
int hat_upfold_to_planes(const void* x, const void* wpk, const float* bias, float* out, int32_t B, int32_t H, int32_t W, int32_t ldx,
                         float out_scale, float mean_r, float mean_g, float mean_b, int32_t dtype, void* stream);
int hat_upfold_to_u8(const void* x, const void* wpk, const float* bias, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride, int32_t B,
                     int32_t H, int32_t W, int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, float mean_r, float mean_g,
                     float mean_b, int32_t bgr, int32_t dtype, void* stream);
int hat_upfold_to_yuv(const void* x, const void* wpk, const float* bias, const HatYuvSurface* dst, int32_t B, int32_t H, int32_t W,
                      int32_t ldx, int32_t h_out, int32_t w_out, float out_scale, float mean_r, float mean_g, float mean_b,
                      const float* from_rgb12, int32_t dtype, void* stream);

/*
 * Chroma siting.  HatYuvSurface keeps its layout (HAT_ABI_VERSION stays 2): the siting travels beside the surface, as a code
 *     HAT_SITING_CENTER 0   chroma in the middle of its luma block: JPEG, MPEG-1, Y4M C420jpeg — every entry above
 *     HAT_SITING_LEFT 1     on the even luma columns, between the rows: MPEG-2, H.264, HEVC, AV1 4:2:0; all standard 4:2:2
 *     HAT_SITING_TOPLEFT 2  on the even luma columns and rows: BT.2020 / UHD HEVC
 * An axis is CO-SITED where it is subsampled and the siting puts chroma on the even luma sample: x where sub_x = 1 and the
 * siting is 1 or 2, y where sub_y = 1 and the siting is 2.  Every other axis keeps the centre rule, so on a 4:2:2 surface 2 is
 * 1, and on 4:4:4 and grey surfaces every siting is 0: accepted, not refused.  The definition is super_resolution_amd/yuv.py
 * ("Chroma siting": chroma_up, chroma_down), and the results equal it bit for bit.
 *   In.  Source pixel (y', x') after the reflection, s[.][.] the chroma samples in byte units, (ch, cw) the chroma plane's size:
 *     j = x' >> sub_x, j1 = min(j + (x' & 1), cw - 1) if x is co-sited, else j;  i, i1 likewise from y', sub_y, ch;
 *     c = ((s[i][j] + s[i][j1]) + (s[i1][j] + s[i1][j1])) * 0.25 (exact), Cb' = c - 128, then the per-pixel expression.
 *   Out.  From the per-pixel cb / cr terms c of the cropped h_out x w_out pixels, every + rounded to fp32 on its own:
 *     co-sited x: t_r[j] = (c[r][max(2j - 1, 0)] + c[r][2j + 1]) + 2 c[r][2j];  centred x: t_r[j] = c[r][2j] + c[r][2j + 1]
 *     4:2:2, siting 1 / 2:  C = t_r[j] * 0.25 + k[c][3]
 *     4:2:0, siting 1:      C = (t_2i[j] + t_2i+1[j]) * 0.125 + k[c][3]
 *     4:2:0, siting 2:      C = ((t_max(2i-1,0)[j] + t_2i+1[j]) + 2 t_2i[j]) * 0.0625 + k[c][3]
 *     Left and top edges replicate; no tap reads past the crop; the byte / code rule is unchanged.
 * hat_yuv_to_planes_sited / hat_planes_to_yuv_sited take hat_yuv_to_planes' / hat_planes_to_yuv's arguments with the siting
 * after the surface.  They refuse everything those refuse, and a siting outside {0, 1, 2}, with HAT_EINVAL before anything
 * touches the device.  Where the surface makes the siting 0 they forward to the unsited entry: the same launch, the same
 * samples.  conv_last's fused epilogue (hat_conv3x3_to_yuv) has no sited form — its bands and lanes would need a halo column and
 * row — so a sited output is hat_conv3x3_to_planes followed by hat_planes_to_yuv_sited.  Other filters (Lanczos, 3/4 - 1/4
 * vertical linear for centred axes), PAL-DV's alternating-line siting and transfer functions are out of scope.
 */
#define HAT_SITING_CENTER 0
#define HAT_SITING_LEFT 1
#define HAT_SITING_TOPLEFT 2
int hat_yuv_to_planes_sited(const HatYuvSurface* src, int32_t siting, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp,
                            const float* to_rgb12, void* stream);
int hat_planes_to_yuv_sited(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatYuvSurface* dst, int32_t siting, int32_t h_out,
                            int32_t w_out, const float* from_rgb12, void* stream);

/*
 * Packed 4:2:2: what SDI capture cards (UYVY, v210), cameras and UVC devices (YUY2) and 10-bit 4:2:2 decoders (Y210 / Y216)
 * deliver.  One array per frame, luma and chroma interleaved, which no HatYuvSurface describes (there is no luma step, and v210
 * is not byte-addressable), so a packed frame has a descriptor of its own.  Per row of w pixels, w even and >= 2, any h >= 1:
 *     HAT_PACKED_UYVY 0   bytes Cb0 Y0 Cr0 Y1 per pixel pair; depth 8; a row is 2 w bytes
 *     HAT_PACKED_YUY2 1   bytes Y0 Cb0 Y1 Cr0; depth 8; 2 w bytes
 *     HAT_PACKED_Y210 2   little-endian 16-bit words Y0 Cb0 Y1 Cr0; depth 10 / 12 / 16 (16: Y216), msb as in the deep entries
 *                         (Y210 proper is msb = 1); 4 w bytes
 *     HAT_PACKED_V210 3   six pixels in four little-endian 32-bit words, three 10-bit codes each at bits 0-9, 10-19, 20-29:
 *                         Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5; depth 10, msb 0 or 1 and not used; a row is
 *                         128 ceil(w / 48) bytes.  Out: bits 30-31 of every word, the codes of the last group past w and every
 *                         byte from the last group to the end of the row are zero.  In: none of them is read for its value.
 *     base, pitch, bstride   the first byte, the bytes between rows and between the frames of a batch (ignored for B == 1);
 *                         base, pitch and bstride are multiples of the unit's word: 4 bytes, 2 for Y210.  reserved is not read.
 * A packed sample means what the sample of a (sub_x, sub_y) = (1, 0) surface means: the definition is super_resolution_amd/yuv.py
 * (packed_to_planes / planes_to_packed, which ARE the 'i422' functions on the unpacked samples), the arithmetic is the shared
 * code of the planar kernels, and the results equal hat_yuv_to_planes_sited / hat_planes_to_yuv_sited on an I422 surface bit for
 * bit.  siting: HAT_SITING_CENTER or HAT_SITING_LEFT (standard 4:2:2 video is LEFT-sited); HAT_SITING_TOPLEFT means LEFT, as on
 * every 4:2:2 surface.  hat_packed422_to_planes reflect-pads to (Hp, Wp); hat_planes_to_packed422 keeps the top-left h_out x
 * w_out pixels.  The destination is written in whole units (a dword for two 8-bit pixels, 8 bytes for two Y210 pixels, 16 bytes
 * for six v210 pixels), one lane a unit; bytes of a pitched row past the layout's row length are never written.
 * HAT_EINVAL, before anything touches the device (none allocates or synchronises): a null pointer; w or w_out odd or < 2; h < 1;
 * a layout outside 0..3; a depth the layout does not take; msb not 0 / 1; a siting outside {0, 1, 2}; a pitch below the row
 * length; base, pitch or (B > 1) bstride not aligned as above; a bstride that makes the frames of a batch overlap; Hp - h >= h or
 * Wp - w >= w (no reflection), Hp < h, Wp < w, h_out > Hs, w_out > Ws; B, Hp or h_out > 65535.
 * There is NO fused packed epilogue (conv_last, the folded ending, the shuffle heads, hat_lte_query): a packed output is fp32
 * planes followed by hat_planes_to_packed422, like a co-sited output.  Packed 4:4:4 and alpha (AYUV / Y410 / RGBA), 4:1:1, 4:4:0
 * and big-endian words are out of scope.
 */
#define HAT_PACKED_UYVY 0
#define HAT_PACKED_YUY2 1
#define HAT_PACKED_Y210 2
#define HAT_PACKED_V210 3
typedef struct { void* base; int64_t pitch, bstride; int32_t layout, depth, msb, reserved; } HatPackedSurface;
int hat_packed422_to_planes(const HatPackedSurface* src, int32_t siting, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp,
                            const float* to_rgb12, void* stream);
int hat_planes_to_packed422(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatPackedSurface* dst, int32_t siting, int32_t h_out,
                            int32_t w_out, const float* from_rgb12, void* stream);

/*
 * MATLAB-style bicubic imresize (basicsr utils/matlab_functions.py:16-178): the resize the reference makes its low-resolution
 * input with (hat/data/imagenet_paired_dataset.py:59).  The definition, operation by operation, is
 * super_resolution_amd/resize.py; the results equal it bit for bit.
 *
 * Tables.  The CALLER builds them on the host (resize.weights_indices reproduces the reference's fp32 arithmetic bit for bit;
 * the device's linspace, division and floor need not round alike) and passes DEVICE pointers: per axis w[out_len][P] fp32
 * weights and src[out_len][P] int32 source indices, row-major, out_len = ceil(in_len * scale).  src holds indices into the
 * source itself, 0 <= src < in_len: the reference's symmetric copy in front of and behind the image is folded in (position s
 * before the image reads -s - 1, behind it 2 in_len - 1 - s).  The library cannot look into device tables: an index outside
 * the source is the caller's error.  n_table = out_len * P, the number of entries of each table, is checked against the sizes.
 * Accumulation.  out1[c][i][x] = sum_k w_h[i][k] * img[c][src_h[i][k]][x] and out[c][i][j] = sum_k w_w[j][k] *
 * out1[c][i][src_w[j][k]]: the H pass first, k ascending from a zero accumulator, every product and every sum rounded to fp32
 * on its own (no fused multiply-add).  No clamp and no rounding on the fp32 results: a bicubic overshoots [0, 1].
 *
 * hat_imresize_rows            the H pass.  src_u8 != 0: src is (B,h,w,3) uint8 with src_pitch >= 3 w bytes per row and
 *                    src_bstride bytes per sample (ignored for B == 1), value float(byte) / 255.0f exactly (hat_u8_to_planes'
 *                    table), plane c = byte (bgr ? 2 - c : c).  src_u8 == 0: src is (B,3,h,w) contiguous fp32 planes (pitch,
 *                    bstride and bgr ignored).  -> mid: (B,3,oh,w) fp32, the caller's workspace.
 * hat_imresize_cols_to_planes  the W pass from mid (B,3,oh,w) -> dst (B,3,Hp,Wp) fp32 planes, reflect-padded by
 *                    hat_u8_to_planes' rule applied to OUTPUT coordinates: plane pixel (y, x) is resized pixel (y', x'), y' = y
 *                    for y < oh else 2 (oh - 1) - y, likewise x'.  Hp - oh >= oh or Wp - ow >= ow is HAT_EINVAL; Hp = oh, Wp = ow:
 *                    no padding.
 * hat_imresize_cols_to_u8      the W pass -> dst (B,oh,ow,3) uint8 with dst_pitch >= 3 ow and dst_bstride: each value clamped to
 *                    [0, 1], x255, rounded half to even (hat_planes_to_u8's conversion); plane c to byte (bgr ? 2 - c : c).
 * All three check their arguments before they touch the device (sizes against n_table, pitches, the reflect condition); none
 * allocates or synchronises.  No plan records these calls.
 */
int hat_imresize_rows(const void* src, int32_t src_u8, int64_t src_pitch, int64_t src_bstride, int32_t bgr, float* mid, int32_t B,
                      int32_t h, int32_t w, int32_t oh, const float* w_h, const int32_t* src_h, int32_t P_h, int64_t n_table,
                      void* stream);
int hat_imresize_cols_to_planes(const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w, const int32_t* src_w,
                                int32_t P_w, int64_t n_table, float* dst, int32_t Hp, int32_t Wp, void* stream);
int hat_imresize_cols_to_u8(const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w, const int32_t* src_w,
                            int32_t P_w, int64_t n_table, uint8_t* dst, int64_t dst_pitch, int64_t dst_bstride, int32_t bgr,
                            void* stream);


/*
 * PSNR / SSIM of two 8-bit frames on the device, with the definitions of the reference's validation loop (basicsr
 * metrics/psnr_ssim.py calculate_psnr / calculate_ssim / _ssim, metrics/metric_util.py to_y_channel).  a, b: (B,h,w,3) uint8
 * with row pitches >= 3 w bytes and sample strides in bytes (ignored for B == 1), as hat_u8_to_planes takes them.
 * crop_border pixels come off every side first (0 crops nothing).  flags: HAT_METRICS_PSNR and / or HAT_METRICS_SSIM select
 * what is produced (at least one); HAT_METRICS_Y scores the BT.601 Y value of each pixel (float32(v) / 255 per channel,
 * y = 65.481 r + 128.553 g + 24.966 b + 16 in fp64, float32(y / 255) * 255 in fp32, not rounded to a level), with
 * HAT_METRICS_BGR naming the byte order of BOTH frames; without HAT_METRICS_Y the three byte values are scored as they are
 * (byte order does not matter then: the flag is ignored).
 *
 * sums: [B][4] doubles in device memory.  sums[b][0] = the sum of squared differences over the cropped frame (all three
 * channels without HAT_METRICS_Y; exact there: accumulated in 64-bit integers), sums[b][1 + c] = the sum of the SSIM map of
 * channel c over its (h - 2 crop - 10) x (w - 2 crop - 10) positions (VALID 11x11 Gaussian window, sigma 1.5, C1 = (0.01 *
 * 255)^2, C2 = (0.03 * 255)^2; only c = 0 with HAT_METRICS_Y).  Entries that are not produced are written as 0.  The caller
 * divides and takes the logarithm: PSNR = 10 log10(255^2 n / sums[0]), SSIM = mean over channels of sums[1 + c] / positions.
 * All SSIM arithmetic is fp64 (sigma^2 = blur(a^2) - mu^2 cancels; fp32 is 4e-4 off on a nearly flat image).  The sums are
 * reproducible bit for bit: per-workgroup partials in `workspace`, added in a fixed order by a second small launch; no
 * floating-point atomics.
 *
 * hat_u8_metrics_workspace_bytes is a pure host query: the size `workspace` must have (8-byte aligned device memory; its
 * content before the call does not matter).  Both functions return HAT_EINVAL for B, h or w < 1, a negative crop_border,
 * unknown flag bits, neither metric selected, a cropped frame without pixels, a cropped frame smaller than 11x11 with
 * HAT_METRICS_SSIM, and more than 65535 sample-channels; hat_u8_metrics also for null pointers, a pitch below 3 w and
 * overlapping samples.  The checks come before anything touches the device; neither function allocates or synchronises.
 */
enum { HAT_METRICS_Y = 1, HAT_METRICS_BGR = 2, HAT_METRICS_PSNR = 4, HAT_METRICS_SSIM = 8 };
int hat_u8_metrics_workspace_bytes(int32_t B, int32_t h, int32_t w, int32_t crop_border, int32_t flags, int64_t* bytes);
int hat_u8_metrics(const uint8_t* a, int64_t a_pitch, int64_t a_bstride, const uint8_t* b, int64_t b_pitch, int64_t b_bstride,
                   int32_t B, int32_t h, int32_t w, int32_t crop_border, int32_t flags, double* sums, void* workspace, void* stream);

/*
 * The ESC-LTE benchmark loop's two device pieces (ESC/esc_arb/test.py eval_psnr; csrc/hat_pil_resize.hip).
 *
 * hat_pil_resize_u8: Pillow's 8-bit bicubic Image.resize (libImaging/Resample.c), which the reference's dataset wrappers make
 * their LR images with (esc_arb/datasets/wrappers.py:149-152).  src: one (h,w,3) uint8 frame with src_pitch >= 3 w bytes per
 * row; dst: (oh,ow,3) uint8 with dst_pitch >= 3 ow (bytes past 3 ow of a row are not touched); mid: 3 ow h bytes of the
 * caller's workspace, the uint8 image between the passes.  Any sizes >= 1, shrinking or enlarging, each axis on its own.
 * Tables.  The CALLER builds them on the host (resize.pil_tables: Pillow's float64 arithmetic) and passes DEVICE pointers,
 * per axis coef[out_len][K] int32 (22-bit fixed point) and bounds[out_len][2] int32 = (first tap, tap count <= K); K = 2
 * ceil(2 max(in / out, 1)) + 1, any size.  Arithmetic.  out = clip8((2^21 + sum_k coef[k] * pixel[first + k]) >> 22) in
 * int32, the horizontal pass (w -> ow) into mid first, then the vertical pass (h -> oh): Pillow's order, and the rounding
 * of mid to bytes is part of the definition.  The result equals PIL.Image.resize((ow, oh), BICUBIC) bit for bit.  The
 * library cannot look into device tables: an entry whose taps leave the source contributes nothing (no read outside src or
 * mid follows from a wrong table), and tables shorter than out_len rows are the caller's error.  HAT_EINVAL for null
 * pointers, a size or K below 1 and a pitch below the row.  Two launches; nothing allocates or synchronises.
 *
 * hat_arb_psnr: utils.py:132-149 (calc_psnr) of an fp32 prediction against an 8-bit ground truth.  pred: (3,ph,pw) contiguous
 * fp32 planes, ph >= h, pw >= w: the top-left (h, w) is scored (test.py:112).  gt: (h,w,3) uint8 with gt_pitch >= 3 w, value
 * float(byte) / 255.0f exactly.  Per pixel d_c = min(max(pred_c, 0), 1) - gt_c in fp32; gray != 0 ('benchmark'): v = (d_0 k_0 +
 * d_1 k_1) + d_2 k_2 with k = float32(65.738, 129.057, 25.064) / 256, every product and sum rounded to fp32 on its own, one
 * term v^2 per pixel; gray == 0 ('div2k', or no eval_type): three terms d_c^2.  shave pixels come off every side (the caller
 * passes S for 'benchmark-S', S + 6 for 'div2k-S').  The squares are formed and added in fp64.  sums: two doubles in device
 * memory, sums[0] = the sum, sums[1] = the number of terms; PSNR = -10 log10(sums[0] / sums[1]) is the caller's.  One partial
 * per workgroup in `workspace`, added in a fixed order by a second small launch: reproducible bit for bit, no atomics.
 * hat_arb_psnr_workspace_bytes is a pure host query of the workspace's size (8-byte aligned device memory).  Both return
 * HAT_EINVAL for h or w < 1, a negative shave and 2 shave >= h or w; hat_arb_psnr also for null pointers, ph < h, pw < w and a
 * pitch below 3 w.  The checks come before anything touches the device; neither function allocates or synchronises.
 * No plan records these calls.
 */
int hat_pil_resize_u8(const uint8_t* src, int64_t src_pitch, int32_t h, int32_t w, uint8_t* mid, uint8_t* dst, int64_t dst_pitch, int32_t oh,
                      int32_t ow, const int32_t* coef_w, const int32_t* bounds_w, int32_t K_w, const int32_t* coef_h,
                      const int32_t* bounds_h, int32_t K_h, void* stream);
int hat_arb_psnr_workspace_bytes(int32_t h, int32_t w, int32_t shave, int64_t* bytes);
int hat_arb_psnr(const float* pred, int32_t ph, int32_t pw, const uint8_t* gt, int64_t gt_pitch, int32_t h, int32_t w, int32_t gray,
                 int32_t shave, double* sums, void* workspace, void* stream);

/*
 * (Shifted-)window self-attention, (S)W-MSA — SURVEY §8 row f2.  Replaces, for one attention branch of a Swin / upstream-HAT
 * block, ESC/basicsr/archs/swinir_arch.py:291-317 (torch.roll by -shift, window_partition, WindowAttention core :147-168
 * with the relative-position bias :153-156 and the shift mask of calculate_mask :262-280, window_reverse, torch.roll by
 * +shift); the same buffers this fork's HAT still registers (hat_arch.py:770-781, 805-818).  The two Linear layers
 * (qkv :146, proj :169) are hat_linear launches on either side.
 * q: (B,H,W,ldq) T, already multiplied by head_dim^-0.5; kv: (B,H,W,ldkv) T with k at channel 0 and v at channel C (for
 * a packed qkv map of row stride 3C: q = base, kv = base + C); head h owns channels [h*d, (h+1)*d), d = C/heads even, <= 32.
 * bias_flip: [heads][(2ws-1)^2] fp32 with bias_flip[h][i] = relative_position_bias_table[(2ws-1)^2 - 1 - i][h]
 * (the kernel indexes by key - query offsets, the reference's relative_position_index by query - key).
 * shift: 0 (W-MSA) or a multiple of 4 below ws (SW-MSA; the reference uses ws/2): windows are taken on the cyclically
 * shifted frame and pairs in different mask bands get -100 added to the logit (not -inf), as in the reference.
 * out: (B,H,W,ldo) T at the un-shifted pixel positions.  ws in {8, 16}; H, W multiples of ws.
 * Pad channels (>= C of q, >= 2C of kv) are never read and those of out never written; q, kv and out need element alignment only
 * (the tuned bf16 kernels for head_dim 24 / 30 at ws 16 are taken when strides and pointers allow their wider accesses).
 */
int hat_window_attention(const void* q, const void* kv, const float* bias_flip, void* out, int32_t B, int32_t H,
                         int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t shift, int32_t ldq, int32_t ldkv,
                         int32_t ldo, int32_t dtype, void* stream);

/*
 * Fused HAB feed-forward half (hat_arch.py:237 with :107-119):
 *     t_out = t_in + fc2( a * SiLU(g) ),  [a | g] = dwconv3x3( fc1( LayerNorm2(t_in) ) )
 * in ONE kernel: the 4C-wide intermediate never leaves the CU (LDS), HBM traffic is one read and one
 * write of the fp32 residual stream.  Optionally also emits the NEXT block's LayerNorm of t_out
 * (n_out, T) and its ESC global-average-pool partials (gap_out[b][tile][16]), saving that pass.
 * t_out must not alias t_in (3x3 halo).  Weights are "fragment packed" by the host:
 *   w1f [chunk][4][KS][64 lanes][8]  : fc1 rows {a: 32c..32c+31, g: hid_p+32c..} of chunk c, MFMA A-fragment order,
 *                                      K = round_up(C+1, 32) with the fc1 BIAS stored as column k = C
 *   w2f [chunk][nt][64 lanes][8]     : fc2 columns 32c..32c+31, k order (g, j<4) -> 4g+j, (g, j>=4) -> 16+4g+j-4
 *   dww [chunk][64 lanes][4 groups x 5 tap pairs] (fp32, or a bf16 duplicated in both halves of a dword): the
 *        depthwise weight of channel (lane & 15) of each 16-channel group {a0, a1, g0, g1} for tap
 *        2*pair + (lane >> 5) — "tap 9" is the depthwise BIAS — zero in lanes with
 *        ((lane & 15) >> 3) != ((lane >> 4) & 1); the kernel expands it to a diagonal MFMA operand
 *   b2 : [nt*16] fp32; hid_p = 32*chunks >= hidden, zero padded.  (b1, dwb: [2*hid_p] fp32 copies of the biases
 *   that are folded into w1f / dww; kept for reference, not read by the kernel.)
 * Spatial tile = (2*waves) rows x 16 columns; hat_ffn_tiles() returns the tile count (leading dim of gap_out).
 */
typedef struct HatFfnDesc {
    const float* t_in;
    float* t_out;
    const float* ln_g;
    const float* ln_b;
    const void* w1f;
    const float* b1;
    const void* dww;
    const float* dwb;
    const void* w2f;
    const float* b2;
    const float* ln1_g;  /* optional fused next LayerNorm (NULL: off) */
    const float* ln1_b;
    void* n_out;         /* (B,H,W,ldn) T */
    float* gap_out;      /* optional [B][tiles][16] */
    int32_t B, H, W, C;
    int32_t chunks;      /* hid_p / 32 */
    int32_t ldn, gap_c;
    int32_t dtype;
    /* optional: LayerNorm2(t_in) already computed by the producer (hat_linear's ln_out with ln_ones): T rows of
     * ldm_in >= 32*ceil((C+1)/32) elements = [LN (C) | 1.0 | zeros].  The kernel then copies instead of normalising
     * (ln_g / ln_b are ignored). */
    int32_t ldm_in;
    const void* m_in;
    /* optional (hat_ffn2 / hat_hab_tail, with ln1_g): also write channels [0, 16) of n_out as a compact (B,H,W,16) T plane —
     * what the next block's ESC 13x13 conv reads (32 contiguous bytes per pixel instead of 32 out of every ldn * 2) */
    void* n16_out;
} HatFfnDesc;

int hat_ffn_tiles(const HatFfnDesc* d, int32_t* tiles_out);
int hat_ffn(const HatFfnDesc* d, void* stream);

/*
 * Second-generation fused feed-forward half for embed_dim 144 / bf16 (same HatFfnDesc, same tile geometry and outputs as
 * hat_ffn; m_in must be NULL): the hidden tensor lives on chip as FP16 (fc1 accumulators converted round-toward-zero:
 * saturating), the depthwise 3x3 and the gate run as packed-fp16 VALU, fc2 is an fp16 MFMA.  Different packing:
 *   w1f [chunk][4][5][64 lanes][8] bf16 : fc1 rows {a: 32c..32c+31 | gate: hid+32c..} of chunk c, A-fragment order,
 *                                         K = 144 zero padded to 160 (NO bias column)
 *   b1  [chunk][64] fp32                : fc1 bias of the chunk's rows in the same order (the MFMA C operand)
 *   dww [chunk][4 groups][10][16] fp16  : depthwise weights of hidden units 32c+8g..+7 per tap 0..8 and the depthwise
 *                                         BIAS as "tap 9": eight a-unit values then eight gate-unit values
 *   w2f [chunk][9][64 lanes][8] fp16    : fc2 columns 32c..32c+31 in natural k order (k = 8*(lane>>4) + j)
 *   b2  [144] fp32.  dwb is not read.  HAT_EUNSUPPORTED unless C == 144 and dtype == HAT_BF16.
 */
int hat_ffn2(const HatFfnDesc* d, void* stream);

/*
 * The whole second half of a HAB (hat_arch.py:233-237 with esc_arch.py:123) in ONE kernel, embed_dim 144 / bf16:
 *     tB    = t + W_aggr . [y16 | n[16:]] + wf . im2col3x3(c1) + bias_b        (= hat_aggr_cab, kept in registers / LDS)
 *     t_out = tB + fc2( a * SiLU(g) ),  [a | g] = dwconv3x3( fc1( LayerNorm2(tB) ) )   (= hat_ffn2)
 * `ffn` as for hat_ffn2 except that ffn.t_in is the residual stream BEFORE the aggregation (t); the fp32 tB that
 * hat_aggr_cab would write and hat_ffn2 read back (with its halo) never exists in memory: 1 152 of the pair's 2 896
 * algorithmic bytes per pixel.  The aggregation is evaluated on the haloed tile (10 x 18 pixels for 8 x 16 outputs).
 * n: (B,H,W,ldn_in) T = LayerNorm1(t) whose first 16 channels are replaced by y16 (B,H,W,16) T; c1 (B,H,W,8) T;
 * w_aggr: the aggregation weights fragment packed as for hat_linear (nt = 9, K = 160); wf, bias_b: hat_cab_fold's outputs.
 */
typedef struct HatHabTailDesc {
    HatFfnDesc ffn;
    const void* n;
    const void* y16;
    const void* c1;
    const void* w_aggr;
    const void* wf;
    const float* bias_b;
    int32_t ldn_in;
    /* hat_hab_tail3 at embed_dim 180 only (c1 / wf unused there): the CAB expand conv's output map and its per-sample scale */
    int32_t ldr2;               /* row stride of r2 (elements) */
    const void* r2;             /* (B,H,W,ldr2) T: c2 = conv3x3(c1) + b2 */
    const float* r2scale;       /* [B][r2scale_bstride] fp32: conv_scale * ECA(c2); 1 KiB must be readable from every sample's row */
    int32_t r2scale_bstride;
    int32_t reserved1;          /* hat_hab_tail3 at embed_dim 144: bit 0 = ffn.t_in, bit 1 = ffn.t_out are FP16 rows (B,H,W,C) instead of
                                 * fp32 ones (a 16-bit residual stream between the blocks of a group; values are clamped to the finite
                                 * FP16 range when written); 0 everywhere else */
} HatHabTailDesc;
int hat_hab_tail(const HatHabTailDesc* d, void* stream);

/*
 * Third generation of the same launch (same HatHabTailDesc, same arithmetic, tiles, outputs and rounding points as
 * hat_hab_tail; replaces the same reference lines).  LayerNorm2(tB) of the haloed tile stays in the REGISTERS of the wave
 * that computed it (fc1 B fragments), and the weights of the current 32 (+32 gate) hidden units are copied into LDS once
 * per workgroup by LDS-DMA and shared by its four waves, instead of every wave streaming its own fragments through L1/L2
 * (344 KB of weights per 8 x 16 tile instead of 1 460 KB).  Different packing of the three per-chunk records:
 *   w1f [chunk][4][5][64 lanes][8] bf16 : as for hat_ffn2, but K = 144 + the fc1 BIAS as column k = 144 (the kernel keeps
 *                                         a 1.0 in k-slot 144 of every pixel inside the image and 0 outside: a pixel the
 *                                         depthwise conv must see as zero padding gets U = 0 exactly, hat_arch.py:112-114)
 *   dww [chunk][1024] fp16              : hat_ffn2's 640-element record zero padded to 2 KiB (two whole LDS-DMA pieces)
 *   w2f [chunk][9][64 lanes][8] fp16    : as for hat_ffn2.   b1 and dwb are not read.
 * embed_dim 180 (HAT / HAT-L; ffn.C == 180, ffn.chunks == 12: the hidden width 360 zero padded to 384): 12 channel tiles, K = 180
 * in 6 k-steps with the fc1 bias as column k = 180 — w1f [12][4][6][64][8], w2f [12][12][64][8], dww [12][1024], b2 a 1 KiB
 * record — and no folded CAB (their squeeze is 60 channels wide): tB = t + W_aggr . [y16 | n[16:]] + r2scale * r2 + bias_b with
 * w_aggr fragment packed [12][6][64][8], bias_b a 1 KiB record [256] (zero padded), r2 / r2scale as below; c1 and wf are ignored.
 */
int hat_hab_tail3(const HatHabTailDesc* d, void* stream);
/*
 * hat_hab_tail3 with the FP16-range guard: hat_conv_guarded's contract for an FP16 t_out (reserved1 bit 1, embed_dim 144).  The
 * values watched are the fp32 t_out of the pixels inside the image, before the clamp; the LayerNorm rows, the compact copy and
 * the pool partials are not part of it (they are computed from the unclamped values anyway).  sat == NULL: hat_hab_tail3.
 * With sat set: reserved1 bit 1 clear, embed_dim 180 (which has no FP16 stream) or a misaligned sat return HAT_EINVAL.
 */
int hat_hab_tail3_guarded(const HatHabTailDesc* d, uint32_t* sat, void* stream);

/*
 * Forward plans — the whole network behind three calls, for hosts without Python (SURVEY §8b's hat_forward(handle ...)).
 * A plan file holds ONE input shape's complete forward: every call of this header in launch order with its descriptors
 * and scalars, every device pointer as (buffer, offset), the packed weights and constants with their bytes, and the sizes
 * of the workspace buffers.  `python -m super_resolution_amd.plan -opt x.yml --shape B H W -o net.hatplan` (or
 * `super_resolution_amd.plan.export_plan(net, shape, path)`) writes it by recording what the engine launches.
 *   hat_plan_load     reads and checks the WHOLE file on the host, then allocates (hipMalloc) and uploads; *out owns the device
 *                     memory.  The file is untrusted input: a refused file has made no device call and allocated nothing on
 *                     the device.  HAT_EUNSUPPORTED: another HAT_ABI_VERSION, another function table size, more than 2^20
 *                     buffers or 2^24 calls.  HAT_EINVAL: no such file, wrong magic, a file that ends early or goes on after
 *                     the last call; B, Cin, H, W, scale or Cout < 1, a dtype other than HAT_F32 / HAT_BF16, a non-zero
 *                     reserved word, scale*H or scale*W past int32, B*3*H*W or B*3*(scale*H)*(scale*W) floats past
 *                     INT64_MAX / 4; a buffer kind > 3 or size > 2^38, anything but exactly one input of B*Cin*H*W*4 bytes
 *                     and one output of B*Cout*(scale*H)*(scale*W)*4 bytes, a constant buffer whose bytes the file does not
 *                     hold; a call whose function id is outside the table, whose argument count or any argument kind is not
 *                     the entry point's (pointer, int32, int64, float, descriptor, host array; the stream last and only
 *                     last), an int32 argument that does not fit, a descriptor whose size is not sizeof its struct in this
 *                     header, a fixup whose field offset is not 8-aligned or not wholly inside the descriptor, more than 64
 *                     fixups, a (buffer, offset) whose buffer does not exist or whose offset is past its bytes.  A positive
 *                     value is the hipError_t of a failed hipMalloc / copy.  csrc/hat_plan_parse.h is that check (host-only
 *                     C++); csrc/hat_plan_check.cpp runs it from the command line on machines without a GPU.
 *   hat_plan_info     dims8 = {B, Cin, H, W, scale, Cout, dtype, 0}; number of launches; device bytes held.
 *   hat_plan_forward  x: (B,Cin,H,W) fp32 NCHW in [0,1], y: (B,Cout,scale*H,scale*W) fp32, both device memory of that
 *                     shape; issues the recorded launches on `stream` (one stream; no allocation, no sync).  Results
 *                     are bit-identical to the Python engine's for the same weights.  Not re-entrant per plan (the
 *                     workspace is the plan's): one forward at a time.
 *   hat_plan_free     releases everything.
 *   hat_plan_forward_u8  the same forward from and to 8-bit frames, for a plan with Cin = Cout = 3.  src: (B,h,w,3) uint8
 *                     device memory, rows src_pitch bytes apart, samples h * src_pitch apart; any h <= H, w <= W with
 *                     H - h < h and W - w < w: the frame is reflect-padded to the plan's (H, W) by hat_u8_to_planes.
 *                     dst: (B, scale*h, scale*w, 3) uint8 device memory, rows dst_pitch bytes apart, samples
 *                     scale*h * dst_pitch apart.  flags bit 0: the bytes of a pixel are B, G, R on both sides.  The
 *                     plan keeps an fp32 input staging buffer (B*3*H*W floats) and, unless its last launch is
 *                     hat_conv3x3_to_planes into the output (then hat_conv3x3_to_u8 is issued with the recorded
 *                     arguments and no fp32 image exists), an fp32 output one: the FIRST u8 call allocates them
 *                     (hipMalloc: it synchronises the device once); later calls allocate nothing.  Results are
 *                     bit-identical to HAT.forward_u8 on a frame that pads to (H, W).  hat_plan_forward is unaffected.
 *                     Returns 0, a negative HAT_E* for a refused argument, or — as hat_plan_load does — the positive
 *                     hipError_t of a failed hipMalloc / launch.
 *   hat_plan_forward_yuv420  the same forward from and to 4:2:0 frames: a source frame block of (B, h, w) and a destination
 *                     frame block of (B, scale*h, scale*w) (see "The 4:2:0 frame boundary"), h and w even, with the size rules
 *                     of hat_plan_forward_u8.  It stages with hat_yuv420_to_planes, replays, and ends in
 *                     hat_conv3x3_to_yuv420 (recorded arguments) or, where the plan does not end in hat_conv3x3_to_planes,
 *                     in hat_planes_to_yuv420 of an fp32 staging image.  The staging buffers are the ones
 *                     hat_plan_forward_u8 uses.  Bit-identical to HAT.forward_yuv420; same return values.
 *   hat_plan_forward_yuv420_deep  hat_plan_forward_yuv420 with a sample width on either side: after each block its depth (8:
 *                     bytes, then pitches are what hat_plan_forward_yuv420 takes and msb is not used; 10 / 12 / 16: 16-bit
 *                     words, see the deep 4:2:0 entries) and msb (0 / 1).  8 -> 10 and 10 -> 8 are this one entry.  It
 *                     replays from the recorded conv_last arguments in the same way (hat_conv3x3_to_yuv420p16 for a deep
 *                     destination), stages only in hat_plan_forward_u8's buffers, and needs no new plan file content.
 *                     Bit-identical to HAT.forward_yuv420(depth=, out_depth=); same return values.
 *   hat_plan_forward_yuv  the same forward between two HatYuvSurface descriptions (see "any chroma subsampling"): src holds
 *                     (B, h, w), dst (B, scale*h, scale*w); any input subsampling / depth to any output one (NV12 -> I444,
 *                     grey -> grey, I444 -> grey ...).  Both surfaces are checked in full before anything is enqueued.  It stages
 *                     with hat_yuv_to_planes, replays, and ends in hat_conv3x3_to_yuv or hat_planes_to_yuv by the rule of
 *                     hat_plan_forward_yuv420, in the same staging buffers.  Bit-identical to HAT.forward_yuv.
 *   hat_plan_forward_yuv_sited  hat_plan_forward_yuv with a chroma siting beside each surface (see "Chroma siting").  It
 *                     refuses what hat_plan_forward_yuv refuses and a siting outside {0, 1, 2}; two sitings that the surfaces
 *                     make 0 ARE hat_plan_forward_yuv.  It stages with hat_yuv_to_planes_sited.  Where the destination is
 *                     co-sited, a plan that ends in hat_conv3x3_to_planes replays that launch too, into its fp32 output
 *                     staging image (allocated on the first such call, as under hat_plan_forward_u8), and ends in
 *                     hat_planes_to_yuv_sited; a centre destination ends by the rule of hat_plan_forward_yuv420.  No new plan
 *                     file content.  Bit-identical to HAT.forward_yuv(siting=, out_siting=).
 */
typedef struct hat_plan hat_plan;
int hat_plan_load(const char* path, hat_plan** out);
int hat_plan_info(const hat_plan* plan, int32_t* dims8, int64_t* n_calls, int64_t* device_bytes);
int hat_plan_forward(const hat_plan* plan, const float* x, float* y, void* stream);
void hat_plan_free(hat_plan* plan);
int hat_plan_forward_u8(const hat_plan* plan, const uint8_t* src, int64_t src_pitch, int32_t h, int32_t w, uint8_t* dst,
                        int64_t dst_pitch, int32_t flags, void* stream);
int hat_plan_forward_yuv420(const hat_plan* plan, const uint8_t* src_y, int64_t src_y_pitch, int64_t src_y_bstride, const uint8_t* src_cb,
                            const uint8_t* src_cr, int64_t src_c_pitch, int32_t src_c_step, int64_t src_c_bstride, int32_t h, int32_t w,
                            uint8_t* dst_y, int64_t dst_y_pitch, int64_t dst_y_bstride, uint8_t* dst_cb, uint8_t* dst_cr, int64_t dst_c_pitch,
                            int32_t dst_c_step, int64_t dst_c_bstride, const float* to_rgb12, const float* from_rgb12, void* stream);
int hat_plan_forward_yuv420_deep(const hat_plan* plan, const void* src_y, int64_t src_y_pitch, int64_t src_y_bstride, const void* src_cb,
                                 const void* src_cr, int64_t src_c_pitch, int32_t src_c_step, int64_t src_c_bstride, int32_t src_depth,
                                 int32_t src_msb, int32_t h, int32_t w, void* dst_y, int64_t dst_y_pitch, int64_t dst_y_bstride, void* dst_cb,
                                 void* dst_cr, int64_t dst_c_pitch, int32_t dst_c_step, int64_t dst_c_bstride, int32_t dst_depth,
                                 int32_t dst_msb, const float* to_rgb12, const float* from_rgb12, void* stream);
int hat_plan_forward_yuv(const hat_plan* plan, const HatYuvSurface* src, const HatYuvSurface* dst, int32_t h, int32_t w,
                         const float* to_rgb12, const float* from_rgb12, void* stream);
int hat_plan_forward_yuv_sited(const hat_plan* plan, const HatYuvSurface* src, int32_t src_siting, const HatYuvSurface* dst,
                               int32_t dst_siting, int32_t h, int32_t w, const float* to_rgb12, const float* from_rgb12, void* stream);
/* hat_plan_forward_packed422: the same forward with a packed 4:2:2 surface ("Packed 4:2:2") on either side or on both.  Exactly one
 * of the two pointers of a side is non-NULL (both or neither: HAT_EINVAL), so UYVY -> UYVY, NV12 -> v210 and v210 -> I420 all work.
 * Both surfaces are checked in full before anything is enqueued.  A planar destination keeps its fused ending where
 * hat_plan_forward_yuv_sited has one; a packed destination ends in the fp32 image and hat_planes_to_packed422. */
int hat_plan_forward_packed422(const hat_plan* plan, const HatPackedSurface* src_packed, const HatYuvSurface* src_planar, int32_t src_siting,
                               const HatPackedSurface* dst_packed, const HatYuvSurface* dst_planar, int32_t dst_siting, int32_t h, int32_t w,
                               const float* to_rgb12, const float* from_rgb12, void* stream);

/*
 * Per-channel sums of a channel-last map over the pixel rectangle rows [r0, r1) x columns [c0, c1):
 *     out[b*ldo + ch] = sum x[b][(r*W + c)*ld + ch],  ch < C,  x: T = bf16 / fp32, ld % 4 == 0 with zero pad channels
 * — the global average pools of the path (ECA, hat_arch.py:73; ESC dynamic kernel, esc_arch.py:96,121) when a frame is sharded
 * into row bands and every band contributes the sums of the rows it OWNS; the bands' vectors are then added
 * (hat_add_f32 on one GPU, an RCCL all-reduce across GPUs) and fed to hat_esc_weights / hat_eca_scale as ONE block, to
 * hat_cab_fold as `stats`.  Deterministic: fixed reduction order, cross-workgroup part in fp64.
 * bstride: elements between samples; tmp: [B][64][256] fp32 scratch; counter: [B] uint32, zero before the first call
 * (the kernel leaves it zero).
 */
int hat_rect_sum(const void* x, int32_t dtype, int32_t ld, int32_t C, int32_t W, int32_t r0, int32_t r1, int32_t c0, int32_t c1,
                 int64_t bstride, int32_t B, float* out, int32_t ldo, float* tmp, uint32_t* counter, void* stream);

/*
 * The eight flips / transposes of fp32 planes (the dihedral group of the rectangle), with a scale and an optional accumulate:
 * the data movement of the geometric self-ensemble (basicsr models/sr_model.py:132-178; HATEngine.forward_ensemble).
 *     src: (planes, H, W) fp32, contiguous.   dst: (planes, H', W') fp32, contiguous.
 *     dst[p][T(y, x)] = (accumulate ? dst[p][T(y, x)] : 0) + alpha * src[p][y][x]
 * op = v | h << 1 | t << 2 names the member T_op = t^b2 o h^b1 o v^b0: v reverses the last axis (W), h reverses H, t swaps H and
 * W, applied in that order (member i of the reference's list of eight).  With inverse != 0, T is T_op^-1 (t undone first, then
 * h, then v): ops 5 and 6 (the quarter turns) are each other's inverses, every other member is its own.  (H', W') = (W, H) when
 * the transform contains t, else (H, W); `inverse` does not change that, H and W always describe src.
 * The product and the sum are each rounded to fp32 (no fused multiply-add); no atomics: the result is deterministic, and every
 * element of dst is written exactly once per call.  One launch covers all planes.  Any H, W >= 1 (ragged tiles are handled
 * inside).  HAT_EINVAL before any launch for: a null pointer, op outside 0..7, planes, H or W < 1, planes > 65535, H or W >
 * 65535 * 64 (the grid), and src / dst byte ranges [p, p + 4 planes H W) that overlap (in place is not supported).
 * A C host gets the self-ensemble of a network by putting this call around two plans, one per orientation.
 */
int hat_dihedral_f32(const float* src, float* dst, int32_t planes, int32_t H, int32_t W, int32_t op, int32_t inverse, float alpha,
                     int32_t accumulate, void* stream);

int hat_abi_version(void);
/* name of the architecture the code objects in this library were compiled for ("gfx950") */
const char* hat_target_arch(void);

/*
 * NIQE on the device (basicsr metrics/niqe.py calculate_niqe, convert_to 'y'): the no-reference score of GT-less test sets.
 * The device delivers, per 96 x 96 block and scale, the 25 sums the AGGD fits need; the fits, the mean / covariance over the
 * blocks and the 36 x 36 pseudo-inverse are tiny and stay with the caller in fp64 (super_resolution_amd/niqe.py:
 * features_from_stats, score).  The reference runs in float32 and the kernels follow it step by step (niqe.py's docstring).
 *
 * hat_niqe_workspace_bytes  a pure host query: H96, W96 = the size of the plane after crop_border pixels come off every side
 *     and the rest is cropped to whole 96 x 96 blocks; bytes = room for the four fp32 buffers of one score: the plane and its
 *     / 255 copy (B,H96,W96 each), the resize intermediate (B,H96/2,W96) and the half-size plane (B,H96/2,W96/2).
 * hat_niqe_y_u8  src: (B,h,w,3) uint8 with pitch >= 3 w bytes per row and bstride bytes per sample (ignored for B == 1), as
 *     hat_u8_metrics takes them; bgr: the bytes are B, G, R.  plane (B,H96,W96) fp32 = the BT.601 Y value hat_u8_metrics
 *     forms under HAT_METRICS_Y, ROUNDED half to even (niqe.py:195).  unit: null, or (B,H96,W96) fp32 = float32(plane) / 255,
 *     correctly rounded: what the half-size resize reads.
 * hat_imresize_plane_rows / hat_imresize_plane_cols  the two passes of hat_imresize_* for ONE fp32 plane per sample:
 *     src (B,h,w) -> mid (B,oh,w) -> dst (B,oh,ow), tables as resize.weights_indices makes them, every product and sum
 *     rounded to fp32 on its own, k ascending; dst = the resized value * out_scale (one more fp32 rounding; 1 changes
 *     nothing).  NIQE's second scale is rows(unit), cols(out_scale = 255).
 * hat_niqe_block_stats  plane: (B,h,w) fp32, h and w multiples of block (96, or 48 for the second scale).  window: 49
 *     doubles in HOST memory, the 7 x 7 Gaussian (niqe.gaussian_window()), read before the call returns.  stats:
 *     (B, h / block, w / block, 25) doubles in device memory; entry 5 m + q: map m = n, n roll(n,(0,1)), n roll(n,(1,0)),
 *     n roll(n,(1,1)), n roll(n,(1,-1)) with the roll wrapping inside the block; q = count of negative values, count of positive
 *     values, sum of squares over the negative, over the positive values (each square an fp32), sum of absolute values.
 *     n = (img - mu) / (sigma + 1), mu = conv7x7(img), sigma = sqrt(|conv7x7(img^2) - mu^2|), borders `nearest` at the IMAGE
 *     edge: the 49 taps accumulate in fp64 in raster order, mu and conv(img^2) are rounded to fp32, the rest is fp32; the
 *     sums are fp64.  One workgroup per block, the block resident in LDS; no intermediate plane is written; no atomics, so
 *     the sums are reproducible bit for bit.
 * All return HAT_EINVAL, before anything touches the device, for null pointers (unit excepted), B, h or w < 1, B > 65535, a
 * negative crop_border, fewer than 96 rows or columns after cropping, a pitch below 3 w or overlapping samples, a table length
 * that is not out_len * P, a block other than 96 or 48, h or w that is no multiple of block, and more than 65535 rows of
 * blocks / output rows (the grid).  None allocates or synchronises.
 */
int hat_niqe_workspace_bytes(int32_t B, int32_t h, int32_t w, int32_t crop_border, int32_t* H96, int32_t* W96, int64_t* bytes);
int hat_niqe_y_u8(const uint8_t* src, int64_t pitch, int64_t bstride, int32_t B, int32_t h, int32_t w, int32_t crop_border, int32_t bgr,
                  float* plane, float* unit, void* stream);
int hat_imresize_plane_rows(const float* src, float* mid, int32_t B, int32_t h, int32_t w, int32_t oh, const float* w_h,
                            const int32_t* src_h, int32_t P_h, int64_t n_table, void* stream);
int hat_imresize_plane_cols(const float* mid, int32_t B, int32_t oh, int32_t w, int32_t ow, const float* w_w, const int32_t* src_w,
                            int32_t P_w, int64_t n_table, float out_scale, float* dst, void* stream);
int hat_niqe_block_stats(const float* plane, int32_t B, int32_t h, int32_t w, int32_t block, const double* window, double* stats,
                         void* stream);

/*
 * NAF stem: the NAFNet-style blocks in front of HATX in HybridHATNAF (hybrid_hat_naf_arch.py:16-82), c = 64 or 32 channels
 * (HAT_EUNSUPPORTED otherwise), fp32 or bf16 storage.  One NAFBlock is
 *     u = pw1(x); v = dw3x3(u); g = v[:c] * v[c:]; s = sca(mean_HW(g)); y = x + beta * pw2(g * s)
 *     u2 = ffn1(y); v2 = ffn_dw(u2); g2 = v2[:c] * v2[c:]; out = y + gamma * ffn2(g2)
 * The global pool cuts it into two halves of one shape, 1x1 c -> 2c, depthwise 3x3 (+ bias), gate: hat_naf_half is one half.
 * The depthwise conv zero-pads u: outside the image u is 0, not the 1x1 conv's bias.
 *
 * hat_naf_half  works on tiles of 8 x 16 pixels with a 1-pixel halo, one workgroup per tile (hat_naf_half_tiles(H, W) per
 *   sample).  It first takes the fp32 residual-stream row of every halo pixel
 *     form (a), gprev == NULL:  r = r_in
 *     form (b), gprev != NULL:  r = r_in + Wf . gprev + bf, written to r_out for the tile's own pixels (halo pixels are
 *                               recomputed, not written: r_out must not be r_in)
 *   then u = W1 . r + b1 on the MFMA units (r rounded to T, fp32 accumulation), the depthwise conv and the gate in fp32, and
 *   stores g as T.  w1 == NULL (form (b) only) stops after r_out: the projection that ends the stem.
 *     r_in, r_out  (B,H,W,ldr) fp32, ldr >= C, ldr % 4 == 0; channels >= C are neither read nor written
 *     gprev        (B,H,W,ldg) T, ldg >= C and a multiple of 16 bytes; must not be g_out
 *     wf           T fragments [C/16][C/32][64 lanes][8]: element (t, ks, l, j) = Wf[16 t + (l & 15)][32 ks + 8 (l >> 4) + j];
 *                  sample b reads wf + b * wf_bstride elements (0: one matrix for all; a multiple of 16 bytes)
 *     bf           fp32 [C], sample b reads bf + b * bf_bstride (0 or a multiple of 4)
 *     w1           T fragments [2C/16][C/32][64][8] of the (2C, C) matrix, same element order;  b1 fp32 [2C]
 *     dww          fp32 [9][2C], tap = 3 ky + kx;  dwb fp32 [2C]
 *     g_out        (B,H,W,ldo) T, ldo >= C and a multiple of 16 bytes; channels >= C keep what they held
 *     partials     optional fp32 [B][tiles][C]: slot (b, tile) = the sums of g over the tile's own pixels inside the image,
 *                  taken from the fp32 values before rounding, in a fixed order (no atomics: two runs agree bit for bit).
 *                  Every slot is written.  Needs w1.
 *   All pointers that are read or written as vectors are 16-byte aligned.  HAT_EINVAL, before any launch, for a null or
 *   misaligned pointer the chosen form needs, bad leading dimensions, B, H or W < 1, B > 65535, r_out == r_in,
 *   g_out == gprev, form (a) without w1, partials without w1.
 *
 * hat_naf_fold  one workgroup per sample: mean = sum of the `tiles` partial slots / npix; s = wsca . mean + bsca;
 *   wf[b] = T(beta[o] * w2[o][i] * s[i]) in hat_naf_half's fragment order ([B][C * C] T); bf[b][o] = beta[o] * b2[o]
 *   ([B][C] fp32).  wsca, w2: fp32 [C][C] row major (out, in); bsca, b2, beta: fp32 [C].  The static second fold of a block
 *   (gamma * ffn2) is made by the host packer.  HAT_EINVAL for a null pointer, wf / bf not 16-byte aligned, B, tiles or
 *   npix < 1.
 */
typedef struct HatNafHalfDesc {
    const float* r_in;
    const void* gprev;
    const void* wf;
    const float* bf;
    float* r_out;
    const void* w1;
    const float* b1;
    const float* dww;
    const float* dwb;
    void* g_out;
    float* partials;
    int64_t wf_bstride;
    int32_t bf_bstride;
    int32_t B, H, W, C, ldr, ldg, ldo, dtype;
    int32_t reserved0;
} HatNafHalfDesc;
int hat_naf_half_tiles(int32_t H, int32_t W);
int hat_naf_half(const HatNafHalfDesc* d, void* stream);

typedef struct HatNafFoldDesc {
    const float* partials;
    const float* wsca;
    const float* bsca;
    const float* w2;
    const float* b2;
    const float* beta;
    void* wf;
    float* bf;
    int64_t npix;
    int32_t B, tiles, C, dtype;
} HatNafFoldDesc;
int hat_naf_fold(const HatNafFoldDesc* d, void* stream);

/*
 * ESC: what the ESC network (esc_arch.py:256-386) needs beyond hat_conv / hat_linear / hat_esc_weights / hat_esc_conv13.
 * dim = 64 channels, fp32 or bf16 storage (the fp32 instantiations are the parity path).
 *
 * hat_esc_convffn  ConvFFN (esc_arch.py:148-159) in one launch, on tiles of 8 x 12 pixels with a 1-pixel halo, one workgroup
 *   per tile (hat_esc_convffn_tiles(H, W) per sample):
 *       n = ln_g ? LayerNorm(x; ln_g, ln_b, ln_eps) : x;  h = gelu(W1 n + b1);  h2 = gelu(dw3x3(h) + dwb) + h;
 *       out = W2 h2 + b2 (+ r)
 *   GELU is the erf form.  The depthwise conv zero-pads h: outside the image h is 0, not gelu(b1).  Both 1x1 convs run on the
 *   MFMA units with their operand rounded to T and fp32 accumulation; the depthwise taps are fp32.
 *     x          (B,H,W,ldx) fp32, ldx >= 64, ldx % 4 == 0
 *     ln_g, ln_b fp32 [64], both or neither; ln_eps > 0
 *     hid_p      the hidden width padded to a multiple of 32: 96 (int(64 * 1.25) = 80) or 128; HAT_EUNSUPPORTED otherwise.
 *                Pad units have zero weights and biases everywhere and contribute 0.
 *     w1         T fragments [hid_p/16][2][64 lanes][8]: element (t, ks, l, j) = W1[16 t + (l & 15)][32 ks + 8 (l >> 4) + j]
 *     b1, dwb    fp32 [hid_p];  dww fp32 [9][hid_p], tap = 3 ky + kx
 *     w2         T fragments [4][hid_p/32][64][8] of the (64, hid_p) matrix, same element order;  b2 fp32 [64]
 *     r          optional (B,H,W,ldr) fp32 residual, ldr >= 64, ldr % 4 == 0
 *     out        (B,H,W,ldo): fp32 rows when out_f32 != 0, else T rows (ldo a multiple of 16 bytes); must not be x
 *     partials   optional fp32 [B][tiles][16]: slot (b, tile) = the sums of out's channels 0..15, as stored, over the tile's
 *                pixels inside the image, in a fixed order (no atomics: two runs agree bit for bit) — the block layout
 *                hat_esc_weights reduces (nblk = tiles).  Every slot is written.
 *   Vector-accessed pointers are 16-byte aligned.  HAT_EINVAL, before any launch, for a null or misaligned pointer, bad
 *   leading dimensions, B, H or W < 1, B > 65535, out == x.
 *
 * hat_window_attention_r  window self-attention with 32 x 32 windows whose edge windows read reflected pixels
 *   (esc_arch.py:205-250): the frame (h, w) is taken as reflect-padded on the right and the bottom to multiples of 32; a
 *   window position past the frame reads q, k and v at the pixel it mirrors (the 1x1 to_qkv commutes with the pad), takes
 *   part in the softmax over all 1024 keys as in the reference, and its own output is dropped.  q, kv, out, head layout and
 *   q's pre-multiplication by head_dim^-0.5 as for hat_window_attention; bias: [heads][63 * 63] fp32, the reference's
 *   relative_position_bias as it is, indexed (ky - qy + 31) * 63 + (kx - qx + 31).  ws == 32 and C == 16 heads
 *   (HAT_EUNSUPPORTED otherwise); no shift.  K, V^T and one head's bias table stay in LDS (fp32: 144 KiB, bf16: 80 KiB).
 *   HAT_EINVAL when a pad would not be smaller than the frame side (32 ceil(h / 32) - h > h - 1), as reflect padding requires.
 *
 * hat_esc_layernorm  y = LayerNorm(x) over 64 channels with `eps` as an argument (esc_arch.py:68-86 uses 1e-6; hat_layernorm
 *   is fixed at 1e-5): x (npix, ldx) fp32 -> y (npix, ldy) T.
 *
 * hat_esc_shuffle_add  y[b][c][s yy + i][s xx + j] = rows[b][yy][xx][c s^2 + s i + j] + x[b][c][yy][xx]: the pixel shuffle of
 *   to_img's rows (B,H,W,ld) fp32 plus the repeat_interleave base image (esc_arch.py:384-385) -> (B,3,sH,sW) fp32 planes.
 */
typedef struct HatEscConvFfnDesc {
    const float* x;
    const float* ln_g;
    const float* ln_b;
    const void* w1;
    const float* b1;
    const float* dww;
    const float* dwb;
    const void* w2;
    const float* b2;
    const float* r;
    void* out;
    float* partials;
    float ln_eps;
    int32_t B, H, W, hid_p, ldx, ldr, ldo, out_f32, dtype;
    int32_t reserved0;
} HatEscConvFfnDesc;
int hat_esc_convffn_tiles(int32_t H, int32_t W);
int hat_esc_convffn(const HatEscConvFfnDesc* d, void* stream);
int hat_window_attention_r(const void* q, const void* kv, const float* bias, void* out, int32_t B, int32_t h, int32_t w,
                           int32_t C, int32_t heads, int32_t ws, int32_t ldq, int32_t ldkv, int32_t ldo, int32_t dtype,
                           void* stream);
int hat_esc_layernorm(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx,
                      int32_t ldy, int32_t dtype, void* stream);
int hat_esc_shuffle_add(const float* rows, const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t s, int32_t ld,
                        void* stream);

/*
 * ESCReal: what ESCReal (esc_real_arch.py:402-475) needs beyond ESC's launches.  DESIGN.md 4.15.
 *
 * hat_escreal_skip  out = [r +] skip(x), skip = Conv2d(3, 128, 1) -> depthwise Conv2d(128, 128, 7, padding 3, reflect) ->
 *   LeakyReLU(0.2) -> Conv2d(128, 64, 1) (esc_real_arch.py:460-465), in one launch, 64 pixels per workgroup.
 *   (1) A 1x1 conv commutes with reflect padding: the hidden map at a pad position is the hidden map at the mirrored pixel, so
 *       x is gathered at (reflect(y), reflect(x)) and no padded copy exists.
 *   (2) Reflect padding puts all 49 taps of every pixel inside, so the first two layers are one dense 7x7 conv 3 -> 128 with
 *       weights dw[c][tap] * W0[c][ci] and the constant bias b0[c] * sum_tap dw[c][tap] + bdw[c] (packing.escreal_skip_fold).
 *   Both GEMMs run on the MFMA units, operands rounded to T, fp32 accumulation; the 128-wide map stays in LDS.
 *     x      (B,3,H,W) fp32 planes
 *     w1     T fragments [8][5][64 lanes][8] of the (128, 160) matrix, column k = 3 tap + ci (tap = 7 ky + kx), k >= 147 zero:
 *            element (t, ks, l, j) = Wf[16 t + (l & 15)][32 ks + 8 (l >> 4) + j];  b1 fp32 [128]
 *     w3     T fragments [4][4][64][8] of the (64, 128) matrix, same element order;  b3 fp32 [64]
 *     r      optional (B,H,W,ldr) fp32 rows added to the result, ldr >= 64, ldr % 4 == 0
 *     out    (B,H,W,ldo) fp32 rows, ldo >= 64, ldo % 4 == 0
 *   HAT_EINVAL, before any launch: a null or misaligned pointer (16 bytes; x: 4), bad leading dimensions, H or W < 4 (reflect
 *   pad 3 needs a side of at least 4), B < 1 or > 65535, an unknown dtype.
 *
 * hat_dysample  the gather of DySample (esc_real_arch.py:361-399; groups 4, end_conv 64 -> 3) with end_conv moved in front of
 *   the (linear) bilinear sampling.  rows (B,H,W,ld) fp32 hold per LR pixel [offset(x) 8 s^2 | scope(x) 8 s^2 | proj 12]:
 *   offset includes its bias, scope has none, proj[3 grp + o] = sum_c end_conv.weight[o][16 grp + c] x[16 grp + c].  Entry
 *   d 4 s^2 + grp s^2 + i s + j of offset / scope / init_pos is axis d (0: x, 1: y) of group grp at output pixel
 *   (s y + i, s x + j): the reference's view(B, 2, -1, H, W), pixel_shuffle(s), view(B, 2, 4, sH, sW).  Per output pixel and
 *   group: off = offset * sigmoid(scope) * 0.5 + init_pos; the grid value 2 (c + 0.5 + off) / size - 1 is un-normalised as
 *   grid_sample(align_corners=False) does and clamped to [0, size - 1] (padding_mode='border'); the four corners are blended;
 *   y[b][o][Y][X] = bias[o] + the sum over the groups.  y: (B,3,sH,sW) fp32 planes.  A sample may lie anywhere in the frame.
 *   s in 2..4 (HAT_EUNSUPPORTED otherwise); HAT_EINVAL for null pointers, B, H, W < 1, ld < 16 s^2 + 12.
 */
int hat_escreal_skip(const float* x, const void* w1, const float* b1, const void* w3, const float* b3, const float* r, float* out,
                     int32_t B, int32_t H, int32_t W, int32_t ldr, int32_t ldo, int32_t dtype, void* stream);
int hat_dysample(const float* rows, const float* init_pos, const float* bias, float* y, int32_t B, int32_t H, int32_t W, int32_t s,
                 int32_t ld, void* stream);

/*
 * ESCRealM: what ESCRealM (esc_real_arch.py:478-661) needs beyond ESCReal's launches.  DESIGN.md 4.18.  The heads of UniUpsample
 * run on hat_conv (HAT_ACT_LRELU is nn.LeakyReLU()'s 0.01, HAT_ACT_LRELU02 the 0.2; HAT_O_PIXSHUF_T with ps_r 2 or 3),
 * hat_conv3x3_to_planes, hat_linear and hat_dysample as they are.
 *
 * hat_unshuffle_pad  check_img_size and PixelUnshuffle(f) of the stem (esc_real_arch.py:606-620, 645-648) in one pass:
 *   rows[b][yb][xb][c f^2 + f i + j] = x[b][c][refl(f yb + i)][refl(f xb + j)], refl(v) = v < size ? v : 2 size - 2 - v (reflect
 *   padding on the right and bottom up to a multiple of f).  x (B,3,h,w) fp32 planes -> rows (B, ceil(h/f), ceil(w/f), ld) fp32,
 *   ld >= 3 f^2; columns >= 3 f^2 of a row are not written.  f is 2 or 4 (HAT_EUNSUPPORTED otherwise).  HAT_EINVAL: a null
 *   pointer, x == rows, B, h, w < 1, ld < 3 f^2, a pad that is not smaller than the side ((f - h % f) % f > h - 1).
 *
 * hat_escrealm_skip  out = [r +] skip(x) for the unshuffled stem: Conv2d(cin, 128, 1) -> depthwise Conv2d(128, 128, 7, padding 3,
 *   reflect) -> LeakyReLU(0.2) -> Conv2d(128, 64, 1), cin = 12 or 48 (HAT_EUNSUPPORTED otherwise), one launch, 8 x 8 pixels per
 *   workgroup.  The 14 x 14 halo of x is gathered at the mirrored pixels (a 1x1 conv commutes with reflect padding); the first
 *   1x1 and the depthwise conv run in fp32 on the halo's hidden map, which stays in LDS; the last 1x1 runs on the MFMA units
 *   with operands rounded to T.
 *     x      (B,H,W,ldx) fp32 rows, ldx >= cin, ldx % 4 == 0, 16-byte aligned
 *     w0     fp32 [128][cin], b0 fp32 [128];  dw fp32 [128][49] (tap = 7 ky + kx), bdw fp32 [128]
 *     w3     T fragments [4][4][64 lanes][8] of the (64, 128) matrix, hat_escreal_skip's w3;  b3 fp32 [64], 16-byte aligned
 *     r      optional (B,H,W,ldr) fp32 rows added to the result;  out (B,H,W,ldo) fp32 rows; ldr, ldo >= 64, % 4 == 0
 *   HAT_EINVAL, before any launch: a null or misaligned pointer, bad leading dimensions, H or W < 4, B < 1 or > 65535, out == x,
 *   an unknown dtype.
 *
 * hat_shuffle_planes  y[b][c][s yy + i][s xx + j] = rows[b][yy][xx][c s^2 + s i + j]: PixelShuffle(s) of rows (B,H,W,ld) fp32
 *   into (B,3,sH,sW) fp32 planes (hat_esc_shuffle_add without the base image).  HAT_EINVAL for null pointers, rows == y,
 *   B, H, W < 1, s outside 1..8, ld < 3 s^2.
 */
int hat_unshuffle_pad(const float* x, float* rows, int32_t B, int32_t h, int32_t w, int32_t f, int32_t ld, void* stream);
int hat_escrealm_skip(const float* x, const float* w0, const float* b0, const float* dw, const float* bdw, const void* w3,
                      const float* b3, const float* r, float* out, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t ldx,
                      int32_t ldr, int32_t ldo, int32_t dtype, void* stream);
int hat_shuffle_planes(const float* rows, float* y, int32_t B, int32_t H, int32_t W, int32_t s, int32_t ld, void* stream);

/*
 * ESC-LTE: the head of the arbitrary-scale model (esc_arb/models/lte.py:34-105; the encoder is ESC's launches).  DESIGN.md 4.19.
 *
 * hat_lte_query  one launch per query set: gather + Fourier basis + the 256 -> 256 -> 256 -> 256 -> 3 MLP + area-weighted sum +
 *   bilinear base image.  For a query with coordinate c = (cy, cx) in [-1, 1] and cell (ky, kx) over a feature map of H x W, and for
 *   the four shifts (vy, vx) in the order (-1,-1), (-1,1), (1,-1), (1,1):
 *     1. c' = clamp(c + fp32(v / (H, W) + 1e-6), -1 + 1e-6, 1 - 1e-6)
 *     2. (i, j) = the pixel grid_sample(mode='nearest', align_corners=False) picks: rint(((c' + 1) n - 1) / 2), half to even,
 *        every product and sum rounded on its own as torch rounds them
 *     3. q = the pixel's centre as make_coord gives it: fp32(-1 + 1/n) + fp32(2/n) * i
 *     4. rel = (c - q) * (H, W)
 *     5. f_k = (freq[2k] rel_y + freq[2k+1] rel_x) + (Wp[k][0] ky H + Wp[k][1] kx W),  k < 128
 *     6. the MLP input: coef[0:128] cos(pi f) | coef[128:256] sin(pi f)
 *     7. pred = Linear + ReLU three times, then Linear to 3
 *     8. area = |rel_y rel_x| + 1e-9
 *   out = sum_n pred_n area_{3-n} / sum(area)  +  grid_sample(inp, c, 'bilinear', padding_mode='border', align_corners=False),
 *   then out * out_a + out_b.
 *     coef, freq   fp32 rows [H*W][ldc / ldf] of the 256 coef / freq channels at each feature pixel; ldc, ldf >= 256, % 4 == 0,
 *                  16-byte aligned (the two halves of one 512-wide row are fine)
 *     inp          (3,H,W) fp32 planes, the network's normalised input
 *     phase        fp32 [128][2] (phase.weight), 16-byte aligned
 *     w1, w2, w3   T fragments [16][8][64 lanes][8] of the (256, 256) matrices imnet.layers.{0,2,4}.weight: element (t, ks, l, j) =
 *                  W[16 t + (l & 15)][32 ks + 8 (l >> 4) + j];  b1, b2, b3 fp32 [256], 16-byte aligned
 *     w4, b4       fp32 [3][256] and [3] (imnet.layers.6): the last layer runs in fp32 from the third layer's accumulators
 *   Explicit mode: coord, cell fp32 (Q,2) in (y, x) order, Q >= 1; out (Q,3) fp32 rows; gh, gw, cell_y, cell_x ignored.
 *   Grid mode: coord == cell == NULL; the queries are the pixel centres of a (gh, gw) image, coordinate of row r =
 *     fp32(-1 + 1/gh) + fp32(2/gh) * r (make_coord's operation order), every query with the cell (cell_y, cell_x); out (3,gh,gw)
 *     fp32 planes.  The output is tiled 4 x 8 so that the queries of a workgroup share feature pixels.
 *   dtype HAT_F32: every step in fp32 (sincospi by the device library), the exact path.  HAT_BF16: the three 256 x 256 layers on
 *     v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the basis is computed in fp32 (sin / cos by v_sin_f32 / v_cos_f32 on the
 *     exact fraction of f / 2) and rounded once when it becomes the first layer's operand.
 *   32 queries (128 MLP rows) per workgroup; the last tile may be ragged.  HAT_EINVAL, before any launch: a null or misaligned
 *   pointer, exactly one of coord / cell null, H, W, Q, gh or gw < 1, H W or gh gw > 2^31 - 1, bad leading dimensions, out == inp,
 *   an unknown dtype.
 */
int hat_lte_query(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                  const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3, const float* b3,
                  const float* w4, const float* b4, const float* coord, const float* cell, int64_t Q, int32_t gh, int32_t gw,
                  float cell_y, float cell_x, float out_a, float out_b, float* out, int32_t dtype, void* stream);

/*
 * hat_lte_query_u8, hat_lte_query_yuv  hat_lte_query's grid mode with another sink: the same queries, the same fp32
 *   image value v * out_a + out_b per channel, but no fp32 image is written.  A workgroup's 4 x 8 tile of output pixels is held by 32
 *   lanes of one wave, which convert and store it.  Arguments up to b4, gh, gw, cell_y, cell_x, out_a, out_b and dtype: hat_lte_query's,
 *   with its refusals.
 *     hat_lte_query_u8   dst (gh, gw, 3) interleaved bytes, rows dst_pitch >= 3 gw bytes apart: hat_planes_to_u8's conversion (clamp to
 *                        [0, 1], x255 in fp32, round half to even); bgr != 0 swaps bytes 0 and 2.  No alignment is asked of dst.
 *     hat_lte_query_yuv  dst one HatYuvSurface of a (gh, gw) frame (B = 1), any subsampling or grey, 8 / 10 / 12 / 16 bits, msb either
 *                        way, centre-sited, checked as hat_planes_to_yuv checks it; from_rgb12 as there.  Per pixel and per chroma
 *                        sample the conversion is hat_planes_to_yuv's, bit for bit: the pair and block sums are taken between lanes
 *                        (lane ^ 1, lane ^ 8; a tile's origin is even in both axes).  A co-sited output needs a halo a tile does not
 *                        have: write planes with hat_lte_query and convert with hat_planes_to_yuv_sited.
 *   HAT_EINVAL, before any launch: what hat_lte_query refuses; a null dst (or dst->y) or from_rgb12; a pitch below the row; gw odd where
 *   the surface subsamples horizontally, gh odd where vertically; a destination plane that overlaps inp.
 */
int hat_lte_query_u8(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                     const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3, const float* b3,
                     const float* w4, const float* b4, int32_t gh, int32_t gw, float cell_y, float cell_x, float out_a, float out_b,
                     uint8_t* dst, int64_t dst_pitch, int32_t bgr, int32_t dtype, void* stream);
int hat_lte_query_yuv(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                      const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3, const float* b3,
                      const float* w4, const float* b4, int32_t gh, int32_t gw, float cell_y, float cell_x, float out_a, float out_b,
                      const HatYuvSurface* dst, const float* from_rgb12, int32_t dtype, void* stream);

/*
 * ESCFP: what ESCFP (esc_fp_arch.py:247-355; 48 channels, 3 heads of 16) needs beyond ESC's launches.  DESIGN.md 4.16.
 * hat_window_attention_r, hat_esc_conv13, hat_conv and hat_linear serve it as they are.
 *
 * hat_escfp_convffn  hat_esc_convffn at 48 channels: the same descriptor, the same contract with 48 wherever that one says 64
 *   (ldx, ldr, ldo >= 48; ln_g, ln_b [48]; b2 [48]; the LayerNorm divides by 48), the same 8 x 12 tiles and pool-partial slots
 *   (hat_esc_convffn_tiles).  Channels >= 48 of a row are neither read nor written.
 *     hid_p   the hidden width padded: 64 (int(48 * 1.25) = 60) or 96 (72 = Block.proj's int(48 * 1.5), and 96);
 *             HAT_EUNSUPPORTED otherwise
 *     w1      T fragments [hid_p/16][2][64 lanes][8] of the (hid_p, 64) matrix W1 zero-padded from 48 to 64 columns (48 is one
 *             and a half k-steps: the x image in LDS is padded with zeros likewise)
 *     w2      T fragments [3][hid_p/32][64][8] of the (48, hid_p) matrix
 *
 * hat_escfp_layernorm  hat_esc_layernorm over 48 channels: x (npix, ldx >= 48) fp32 -> y (npix, ldy >= 48) T, `eps` an argument.
 *
 * hat_escfp_weights  the per-sample weights of DecomposedConvolutionalAttention (esc_fp_arch.py:102-120), pdim 16, 13 x 13:
 *       p = mean over the frame = (fixed-order sum of the nblk pool partials [B][nblk][16]) / npix
 *       dyn = W2 gelu(W1 p + b1) + b2                     W1 (4,16), b1 [4], W2 (144,4) rows 9 o + 3 ky + kx, b2 [144]; erf GELU
 *       K[o][tap] = lk_spatial[o][tap] + (dyn[o] on the central 3 x 3 taps)
 *       w_out[b][o][16 tap + i] = T( lk_channel[o][i] * K[o][tap] )          one fp32 product, rounded once
 *   A 1x1 conv (lk_channel, no bias) followed by a depthwise 13 x 13 with zero padding is this dense 16 -> 16 conv with zero
 *   padding, at the border too.  w_out: (B,16,Kpad) T in the [16][Kpad] row layout hat_esc_conv13 and hat_conv (ksize 13,
 *   w_bstride = 16 Kpad) read; K >= 169 * 16 is written as zeros.  All operands fp32; lk_channel [16][16], lk_spatial [16][169].
 *   No atomics: two runs agree bit for bit.  HAT_EINVAL for a null pointer, B, nblk or npix < 1, Kpad < 2704.
 *
 * hat_escfp_shuffle_bicubic  y[b][c][s yy + i][s xx + j] = rows[b][yy][xx][c s^2 + s i + j] + bicubic_s(x)[b][c][s yy + i][s xx + j]
 *   (esc_fp_arch.py:354): rows (B,H,W,ld) fp32, x (B,3,H,W) fp32 planes, y (B,3,sH,sW) fp32 planes.  bicubic_s is
 *   F.interpolate(scale_factor = s, mode = 'bicubic', align_corners = False): Keys' cubic with A = -0.75 at src = (o + 0.5) / s
 *   - 0.5, so output phase p = o % s has four fixed weights ptab[p][0..3] (fp32 [s][4], 16-byte aligned) on the source taps
 *   o / s + first .. first + 3, first = (2 p + 1 < s) ? -2 : -1, each tap index clamped to the frame: any H, W >= 1 is legal.
 *   No clamp of the result.  s in 2..4 (HAT_EUNSUPPORTED otherwise); HAT_EINVAL for null pointers, B, H, W < 1, ld < 3 s^2.
 */
int hat_escfp_convffn(const HatEscConvFfnDesc* d, void* stream);
int hat_escfp_layernorm(const float* x, void* y, const float* gamma, const float* beta, float eps, int64_t npix, int32_t ldx,
                        int32_t ldy, int32_t dtype, void* stream);
int hat_escfp_weights(const float* partials, int32_t nblk, int64_t npix, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* lk_channel, const float* lk_spatial, void* w_out, int32_t B, int32_t Kpad,
                      int32_t dtype, void* stream);
int hat_escfp_shuffle_bicubic(const float* rows, const float* x, const float* ptab, float* y, int32_t B, int32_t H, int32_t W,
                              int32_t s, int32_t ld, void* stream);

/*
 * The shuffle heads of the ESC family into a frame: PixelShuffle(s) of fp32 rows, plus a base image, stored as
 * bytes or as a YCbCr surface.  No fp32 image is written.  The value of output pixel (b, c, Y, X), Y < s H, X < s W, is
 *     rows[b][Y / s][X / s][c s^2 + (Y % s) s + X % s]  (+ base[b][c][Y / s][X / s] when base is not NULL: one rounded fp32 add)
 * which is what hat_esc_shuffle_add (with base) and hat_shuffle_planes (without) store, and the top-left (h_out, w_out) pixels are
 * converted as hat_planes_to_u8 / hat_planes_to_yuv convert them: the results are those of the two-step composition bit for bit.
 *     rows     (B,H,W,ld) fp32 rows, ld >= 3 s^2;  base  NULL or (B,3,H,W) fp32 planes;  s in 1..8
 *     h_out, w_out   the crop, 1 <= h_out <= s H, 1 <= w_out <= s W
 *
 * hat_shuffle_to_u8   dst (B,h_out,w_out,3) interleaved bytes, rows dst_pitch >= 3 w_out bytes apart, samples dst_bstride bytes apart
 *   (ignored for B == 1); bgr != 0 swaps bytes 0 and 2.  No alignment is asked of dst.
 * hat_shuffle_to_yuv  dst one HatYuvSurface of (B, h_out, w_out) frames, any subsampling or grey, 8 / 10 / 12 / 16 bits, msb either
 *   way, centre-sited, checked as hat_planes_to_yuv checks it; from_rgb12 as there.  A co-sited output is written from planes
 *   (hat_planes_to_yuv_sited).
 * HAT_EINVAL, before any launch: a null rows, dst (or dst->y) or from_rgb12; rows or base not 4-byte aligned; B, H, W, s, h_out or
 *   w_out < 1; B or h_out > 65535; H W > 2^31 - 1; ld < 3 s^2; a crop beyond (s H, s W); a pitch below the row, overlapping samples of a batch, odd
 *   pitches of 16-bit words; w_out odd where the surface subsamples horizontally, h_out odd where vertically.
 * HAT_EUNSUPPORTED: s > 8.
 */
int hat_shuffle_to_u8(const float* rows, int32_t ld, const float* base, int32_t B, int32_t H, int32_t W, int32_t s, uint8_t* dst,
                      int64_t dst_pitch, int64_t dst_bstride, int32_t h_out, int32_t w_out, int32_t bgr, void* stream);
int hat_shuffle_to_yuv(const float* rows, int32_t ld, const float* base, int32_t B, int32_t H, int32_t W, int32_t s,
                       const HatYuvSurface* dst, int32_t h_out, int32_t w_out, const float* from_rgb12, void* stream);

/*
 * SRVGGNetCompact (srvgg_arch.py:6-69): one conv + activation layer of the compact VGG-style generator.
 *     out[b][y][x][n] = f_n( sum over tap, ci of X[b][y + ty - 1][x + tx - 1][ci] * W[n][ci][ty][tx] + bias[n] ),  n < 64,
 *     f_n(v) = v >= 0 ? v : slope[n] * v
 * a 3x3 conv, zero padding 1, stride 1, to 64 channels.  slope (fp32[64]) is always read: the PReLU weight, zeros for ReLU, 0.1
 * for the reference's LeakyReLU.  fp32 accumulation; bias, slope and activation in fp32; one rounding to T at the store.
 *     frame == 0   x (B,H,W,ldx) T rows of 64 channels, ldx >= 64 and rows of whole 16 bytes; K = 9 * 64
 *     frame != 0   x (B,3,H,W) fp32 planes, used as they are (no mean, no scale; converted to T before the MFMA); ldx is ignored;
 *                  K = 27, k = 9 ci + 3 ty + tx, padded to one 32-deep k-step
 *     out          (B,H,W,ldo) T rows, ldo >= 64 and rows of whole 16 bytes; columns >= 64 are not written; out != x
 *     w            packing.pack_vgg_conv's image: MFMA A fragments [slices][k-steps][n-tiles per slice][64 lanes][8] of T, where
 *                  a workgroup owns `slices`' share of the 64 outputs with its weights resident in LDS: bf16 1 slice of 4
 *                  n-tiles (72 KB), fp32 2 slices of 2 (72 KB each; the fp32 tile is 86 KB).  k-step = 2 tap + half for rows.
 *     dtype        HAT_BF16 (the product path) or HAT_F32 (hat_conv's fp32 products: chains of v_mfma_f32_16x16x4_f32)
 * Persistent workgroups of 8 waves walk the 16 x 16 tiles of all samples: tile t of ceil(W/16) ceil(H/16) B goes to workgroup
 * t % wgs of its slice; hat_vgg_conv_tiles reports tiles, wgs (per slice) and slices for a shape, so workgroup i < min(wgs, tiles)
 * takes ceil((tiles - i) / wgs) trips.  HAT_EINVAL, before any launch: a null pointer; x (rows), w, bias, slope or out not 16-byte
 * aligned (x as planes: 4); B, H or W < 1; more than 2^30 tiles; a bad leading dimension; out == x; another dtype.
 */
typedef struct HatVggConvDesc {
    const void* x;
    const void* w;
    const float* bias;
    const float* slope;
    void* out;
    int32_t B, H, W;
    int32_t ldx, ldo;
    int32_t frame;
    int32_t dtype;
    int32_t reserved0;
} HatVggConvDesc;
int hat_vgg_conv(const HatVggConvDesc* d, void* stream);
int hat_vgg_conv_tiles(int32_t B, int32_t H, int32_t W, int32_t dtype, int32_t* tiles, int32_t* wgs, int32_t* slices);

/*
 * RRDBNet (rrdbnet_arch.py:9-119): one 3x3 conv (zero padding 1, stride 1) of a residual dense block on DENSE ROWS.
 * A block's input and its grown maps share one row buffer (B,H,W,ld) of T, ld >= 192: channels [0,64) hold the block's input x,
 * [64 + 32 (k - 1), 64 + 32 k) hold x_k.  No concatenation is ever made.
 *     cin 64, 96, 128, 160 (convs 1-4), cout 32:
 *         out[p][out_off + n] = f(acc[p][n] + bias[n]),  f(v) = v >= 0 ? v : slope * v,  rounded once to T
 *         out may be x itself (the block's own buffer, out_off = cin): the kernel reads channels [0, cin) only, with 16-byte loads
 *         none of which reaches channel cin, and stores channels [out_off, out_off + 32) only, so reads and writes of a launch never
 *         share a byte although other workgroups store while a workgroup still reads its halo.  out == x requires out_off >= cin and
 *         ldo == ldx.  Two DIFFERENT pointers into one buffer are the caller's to keep apart.  r1, r2, s_out must be NULL.
 *     cin 192 (conv 5), cout 64, no activation, the residual arithmetic of :39 and :62 on an fp32 stream:
 *         v = beta1 * (acc + bias) + r1[p][n]             (r1 == NULL: + 0)
 *         v = beta2 * v + r2[p][n]                        (r2 given; needs r1)
 *         s_out[p][n] = v (fp32), out[p][out_off + n] = v rounded once to T
 *         r1, r2, s_out are fp32 rows (B,H,W,64) without padding; s_out may be r1 or r2 (every element is read, then written, by
 *         one lane).  out is the NEXT block's dense buffer (out_off 0), never x.
 *     w      packing.pack_rdb_conv's image: MFMA A fragments [slices][k-steps][2 n-tiles][64 lanes][8] of bf16 with
 *            k-step = 9 (channel / 32) + 3 ty + tx, element (lane l, j) = W[32 slice + 16 t + (l & 15)][32 (channel / 32) + 8 (l >> 4) + j][ty][tx];
 *            1 slice for convs 1-4, 2 for conv 5.  bias fp32[cout].
 *     slope, beta1, beta2   fp32, applied in fp32 after the fp32 accumulation whose initial value is the bias.
 *     dtype  HAT_BF16 (v_mfma_f32_16x16x32_bf16).  HAT_F32 passes the argument checks and returns HAT_EUNSUPPORTED: the fp32
 *            compute path runs these layers on hat_conv.
 * Persistent workgroups of 8 waves keep their 32 outputs' weights in LDS and walk the 16 x 16 tiles of all samples in 64-channel
 * chunks of the haloed tile: tile t of ceil(W/16) ceil(H/16) B goes to workgroup t % wgs of its slice; hat_rdb_conv_tiles reports
 * tiles, wgs (per slice) and slices.  HAT_EINVAL, before any launch: a null pointer; x, w, bias, out, r1, r2 or s_out not 16-byte
 * aligned; cin not in {64, 96, 128, 160, 192}; cout not 32 (64 for cin 192); ldx < cin; ldo < out_off + cout; ldx, ldo or out_off
 * not giving whole 16 bytes; B, H or W < 1; more than 2^30 tiles; r2 without r1; s_out missing at cin 192; a stream pointer at
 * another cin; out == x with out_off < cin or ldo != ldx; another dtype.
 */
typedef struct HatRdbConvDesc {
    const void* x;
    const void* w;
    const float* bias;
    void* out;
    const float* r1;
    const float* r2;
    float* s_out;
    int32_t B, H, W;
    int32_t cin, cout;
    int32_t ldx, ldo, out_off;
    float slope, beta1, beta2;
    int32_t dtype;
} HatRdbConvDesc;
int hat_rdb_conv(const HatRdbConvDesc* d, void* stream);
int hat_rdb_conv_tiles(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t* tiles, int32_t* wgs, int32_t* slices);

#ifdef __cplusplus
}
#endif
#endif /* HAT_MI355X_H */
