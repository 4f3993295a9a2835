// hat_lte.hip — the LTE head (Local Texture Estimator, esc_arb/models/lte.py:34-105) as ONE kernel on gfx950: for a tile of 32
// queries the gather of the four nearest feature pixels, the Fourier basis, the 256 -> 256 -> 256 -> 256 -> 3 MLP on the four
// 32-row groups, the area-weighted sum and the bilinear base image.
//
//   hat_lte_query   explicit mode: coord / cell (Q,2) -> out (Q,3);  grid mode: the make_coord grid of a (gh, gw) image, computed in
//                   the kernel, -> out (3,gh,gw) planes.  Both with the affine out * a + b.
//   hat_lte_query_u8 / hat_lte_query_yuv   grid mode with another sink: the same fp32 image value, stored as interleaved bytes
//                   (hat_unit_to_u8) or as a YCbCr surface of any layout and depth (hat_planes_to_yuv's conversion); no fp32 image.
//
// A workgroup (256 threads, 4 waves) owns 32 queries = 128 MLP rows (row = 32 shift + query).  The rows live in LDS as T
// ([128][LD], the MFMA B operand; T = bf16 or fp32) from the basis to the last hidden layer; a layer's 256 x 256 weights stream
// from L2 as pre-packed A fragments ([16 n-tiles][8 k-steps][64 lanes][8], packing.pack_lte_mlp), wave w owns output channels
// 64 w .. 64 w + 63 of all 128 rows (4 x 8 accumulator tiles), and the layer's output replaces its input in place once every
// wave has finished reading.  The last layer (256 -> 3) is folded into the third layer's epilogue from the fp32 accumulators.
// Grid mode tiles the output 4 x 8 so that the queries of a tile share feature pixels.
// Contract: include/hat_mi355x.h "ESC-LTE".  DESIGN.md 4.19, 4.20.
#include "hat_frame_sink.h"

namespace {

constexpr int LTE_HID = 256, LTE_TQ = 32, LTE_ROWS = 4 * LTE_TQ, LTE_THREADS = 256, LTE_TY = 4, LTE_TX = 8, LTE_KS = LTE_HID / 32;

struct LteArgs {
    const float* coef; const float* freq; const float* inp; const float* phase;
    const void* w[3]; const float* b[3]; const float* w4; const float* b4;
    const float* coord; const float* cell; float* out;
    int64_t Q;
    int H, W, ldc, ldf, gh, gw, tiles_x;
    float cell_y, cell_x;     // grid mode: the cell of every query
    float gy0, gys, gx0, gxs; // grid mode: coordinate of row r = gy0 + gys * r (make_coord's operation order)
    float fy0, fys, fx0, fxs; // centre of feature row i = fy0 + fys * i
    float sy[2], sx[2];       // the shifts (-1 / +1) * (1 / H, 1 / W) + 1e-6, rounded to fp32 once on the host
    float out_a, out_b;
};

template <typename T> struct LteLds {
    static constexpr int LD = lds_row_elems(LTE_HID, sizeof(T));
    static constexpr size_t ACT = (size_t)LTE_ROWS * LD * sizeof(T);
    static constexpr size_t META = (size_t)LTE_ROWS * 6 * sizeof(float) + (size_t)LTE_TQ * 2 * sizeof(float);
    static constexpr size_t PART = (size_t)4 * LTE_ROWS * 3 * sizeof(float);
    static constexpr size_t BYTES = ACT + META + PART;
    static_assert(BYTES <= HAT_LDS_MAX, "tile does not fit in LDS");
};

// The products and sums that decide WHICH feature pixel a query reads are rounded one by one, as torch's are: a fused multiply-add
// would move a coordinate that sits on a cell boundary.
__device__ __forceinline__ float lte_axpy(float a, float s, float i) {
#pragma clang fp contract(off)
    const float p = s * i;
    return a + p;
}
__device__ __forceinline__ float lte_unnormalize(float c, float n) {   // grid_sample, align_corners=False
#pragma clang fp contract(off)
    const float t = (c + 1.0f) * n;
    return (t - 1.0f) / 2.0f;
}
__device__ __forceinline__ float lte_rel(float c, float q, float n) {
#pragma clang fp contract(off)
    const float d = c - q;
    return d * n;
}

template <typename T> __device__ __forceinline__ void lte_sincospi(float f, float& s, float& c) {
    if constexpr (sizeof(T) == 2) {
        // v_sin_f32 / v_cos_f32 take their argument in revolutions: sin(pi f) = v_sin(f / 2).  The halving and the fraction are exact.
        const float t = __builtin_amdgcn_fractf(0.5f * f);
        s = __builtin_amdgcn_sinf(t);
        c = __builtin_amdgcn_cosf(t);
    } else {
        sincospif(f, &s, &c);
    }
}

template <typename T> __device__ __forceinline__ void lte_store2(T* p, float a, float b) {
    if constexpr (sizeof(T) == 2) {
        typedef bf16_t v2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<v2*>(p) = v2{(bf16_t)a, (bf16_t)b};
    } else {
        *reinterpret_cast<f32x2*>(p) = f32x2{a, b};
    }
}

// acc[tt][pt] += W[64 wave + 16 tt ..][:] . act[16 pt ..][:]
template <typename T>
__device__ __forceinline__ void lte_layer(const T* __restrict__ wf, const T* act, int wave, int lane, f32x4 (&acc)[4][8]) {
    typedef typename MT<T>::frag_t frag_t;
    constexpr int LD = LteLds<T>::LD;
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int pt = 0; pt < 8; ++pt) acc[tt][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int ks = 0; ks < LTE_KS; ++ks) {
        frag_t a[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) a[tt] = MT<T>::load(wf + ((size_t)((4 * wave + tt) * LTE_KS + ks) * 64 + lane) * 8);
#pragma unroll
        for (int pt = 0; pt < 8; ++pt) {
            const frag_t bfr = MT<T>::load(act + (16 * pt + l15) * LD + 32 * ks + 8 * g);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[tt][pt] = MT<T>::mma(a[tt], bfr, acc[tt][pt]);
        }
    }
}

// Where the last phase stores a query's three values.  LtePlanes: a.out, planes (grid mode) or rows (explicit mode), the store the
// kernel always had.  The other two are grid mode only: the 32 lanes of a 4 x 8 tile hold the fp32 image value v * out_a + out_b of
// their pixel (lte_pixel) and convert it.
struct LtePlanes {};

// (gh, gw, 3) interleaved bytes, rows `pitch` bytes apart: hat_unit_to_u8 of each value, bytes 0 and 2 swapped with bgr
struct LteU8 {
    uint8_t* dst;
    long long pitch;
    int bgr;
    __device__ __forceinline__ void store(const float (&rgb)[3], bool valid, int oy, int ox) const {
        if (!valid) return;
        uint8_t* o = dst + (size_t)oy * pitch + (size_t)ox * 3;
        o[bgr ? 2 : 0] = (uint8_t)hat_unit_to_u8(rgb[0]);
        o[1] = (uint8_t)hat_unit_to_u8(rgb[1]);
        o[bgr ? 0 : 2] = (uint8_t)hat_unit_to_u8(rgb[2]);
    }
};

// A YCbCr surface, centre-sited: hat_rgb_to_ycc per pixel, then the one-pixel stores of hat_frame_sink.h (yuv_store_luma,
// yuv_store_chroma420 / 422 / 444), which yuv_store_tile of the planes route shares.  The tile origin is even in both axes, so lane
// q's horizontal partner is q ^ 1 and its vertical partner q ^ 8, and the lane with even ox (and even oy where SUB_Y) stores the chroma sample of its pair / block.  store() is called by every lane of the wave, valid or not: the
// exchanges are outside every branch; a lane without a pixel converts zeros and stores nothing.  The subsampled axes of the image
// have even extent (the host checks it), so the partner of a lane that stores is a pixel of the image.
template <typename S, int SUB_X, int SUB_Y, bool GREY> struct LteYuv {
    HatYuvDst<S> d;   // (one image: sample 0)
    HatCsc k;
    HatSample<S> q;
    __device__ __forceinline__ void store(const float (&rgb)[3], bool valid, int oy, int ox) const {
        float Y, cb, cr;
        hat_rgb_to_ycc(k, rgb[0], rgb[1], rgb[2], Y, cb, cr);
        if (valid) yuv_store_luma(d, q, 0, oy, ox, Y);
        if constexpr (!GREY) {
            if constexpr (SUB_X == 1) {
                // the pair sum left + right, in that order, on the even lane
                const float sb = hat_add_rn(cb, __shfl_xor(cb, 1)), sr = hat_add_rn(cr, __shfl_xor(cr, 1));
                if constexpr (SUB_Y == 1) {
                    const float bb = __shfl_xor(sb, 8), br = __shfl_xor(sr, 8);   // the bottom row's pair sums, on the top row's lanes
                    if (valid && !(ox & 1) && !(oy & 1)) yuv_store_chroma420(d, q, k, 0, oy >> 1, ox >> 1, sb, bb, sr, br);
                } else {
                    if (valid && !(ox & 1)) yuv_store_chroma422(d, q, k, 0, oy, ox >> 1, sb, sr);
                }
            } else {
                if (valid) yuv_store_chroma444(d, q, k, 0, oy, ox, cb, cr);
            }
        }
    }
};

// One query's three values for the byte and YCbCr sinks: the area-weighted sum with the diagonal swap, plus the bilinear base image
// (border padding), then the affine.                                                                             lte.py:95-104
// The plane store below states this as plain expressions and leaves the fusing of its products and sums to the compiler, and how
// those fuse may differ from one instantiation to the next.  A sink's bytes must be those of the planes, so here the operation
// order the plane store compiles to is written out — contraction off, every fused multiply-add explicit:
//   base = fma(p11, wse, fma(p10, wsw, fma(p00, wnw, p01 * wne))),  v = fma(P3, w3, fma(P2, w2, fma(P0, w0, P1 * w1))),
//   value = fma(v + base, out_a, out_b).
// tests/test_gpu_esclte_frames.py holds the two equal bit for bit; DESIGN.md 4.20.
__device__ __forceinline__ void lte_pixel(const LteArgs& a, int q, const float* m_area, const float* m_cy, const float* m_cx, const float* part,
                                          float (&rgb)[3]) {
#pragma clang fp contract(off)
    const int H = a.H, W = a.W;
    const float a0 = m_area[q], a1 = m_area[LTE_TQ + q], a2 = m_area[2 * LTE_TQ + q], a3 = m_area[3 * LTE_TQ + q];
    const float tot = ((a0 + a1) + a2) + a3;
    const float w0 = a3 / tot, w1 = a2 / tot, w2 = a1 / tot, w3 = a0 / tot;
    const float cy = m_cy[q], cx = m_cx[q];
    float iy = fminf(fmaxf(lte_unnormalize(cy, (float)H), 0.f), (float)(H - 1));
    float ix = fminf(fmaxf(lte_unnormalize(cx, (float)W), 0.f), (float)(W - 1));
    const float fy = floorf(iy), fx = floorf(ix);
    const int y0 = min(max((int)fy, 0), H - 1), x0 = min(max((int)fx, 0), W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ty = iy - fy, tx = ix - fx;
    const float wnw = (1.f - tx) * (1.f - ty), wne = tx * (1.f - ty), wsw = (1.f - tx) * ty, wse = tx * ty;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pl = a.inp + (int64_t)c * H * W;
        const float p00 = pl[(int64_t)y0 * W + x0], p01 = pl[(int64_t)y0 * W + x1], p10 = pl[(int64_t)y1 * W + x0], p11 = pl[(int64_t)y1 * W + x1];
        const float base = __builtin_fmaf(p11, wse, __builtin_fmaf(p10, wsw, __builtin_fmaf(p00, wnw, p01 * wne)));
        const float v = __builtin_fmaf(part[(3 * LTE_TQ + q) * 3 + c], w3,
                                       __builtin_fmaf(part[(2 * LTE_TQ + q) * 3 + c], w2,
                                                      __builtin_fmaf(part[q * 3 + c], w0, part[(LTE_TQ + q) * 3 + c] * w1)));
        rgb[c] = __builtin_fmaf(v + base, a.out_a, a.out_b);
    }
}

template <typename T, typename Sink>
__global__ __launch_bounds__(LTE_THREADS) void lte_query_kernel(const LteArgs a, const Sink sink) {
    typedef LteLds<T> L;
    constexpr int LD = L::LD;
    extern __shared__ __attribute__((aligned(16))) unsigned char lte_smem[];
    T* act = reinterpret_cast<T*>(lte_smem);
    float* m_ry = reinterpret_cast<float*>(lte_smem + L::ACT);
    float* m_rx = m_ry + LTE_ROWS;
    float* m_area = m_rx + LTE_ROWS;
    float* m_ch = m_area + LTE_ROWS;   // cell * (H, W)
    float* m_cw = m_ch + LTE_ROWS;
    int* m_pix = reinterpret_cast<int*>(m_cw + LTE_ROWS);
    float* m_cy = reinterpret_cast<float*>(m_pix + LTE_ROWS);   // the query's own coordinate, per query
    float* m_cx = m_cy + LTE_TQ;
    float* part = m_cx + LTE_TQ;       // [4 waves][128 rows][3]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int H = a.H, W = a.W;
    const bool grid = a.coord == nullptr;
    const int ty0 = grid ? (int)(blockIdx.x / a.tiles_x) * LTE_TY : 0, tx0 = grid ? (int)(blockIdx.x % a.tiles_x) * LTE_TX : 0;
    const int64_t q0 = (int64_t)blockIdx.x * LTE_TQ;

    // ---- per row (shift, query): the nearest feature pixel, rel, area                                      lte.py:51-77, 92-93
    if (tid < LTE_ROWS) {
        const int s = tid >> 5, q = tid & 31;
        float cy = 0.f, cx = 0.f, ky = 0.f, kx = 0.f;
        bool valid;
        if (grid) {
            const int oy = ty0 + q / LTE_TX, ox = tx0 + q % LTE_TX;
            valid = oy < a.gh && ox < a.gw;
            cy = lte_axpy(a.gy0, a.gys, (float)oy);
            cx = lte_axpy(a.gx0, a.gxs, (float)ox);
            ky = a.cell_y;
            kx = a.cell_x;
        } else {
            valid = q0 + q < a.Q;
            if (valid) {
                cy = a.coord[2 * (q0 + q)];
                cx = a.coord[2 * (q0 + q) + 1];
                ky = a.cell[2 * (q0 + q)];
                kx = a.cell[2 * (q0 + q) + 1];
            }
        }
        if (!valid) cy = cx = ky = kx = 0.f;   // a row past the end computes on pixel (0, 0)'s neighbourhood and is dropped
        const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
        const float py = fminf(fmaxf(hat_add_rn(cy, a.sy[s >> 1]), lo), hi), px = fminf(fmaxf(hat_add_rn(cx, a.sx[s & 1]), lo), hi);
        int i = (int)__builtin_rintf(lte_unnormalize(py, (float)H)), j = (int)__builtin_rintf(lte_unnormalize(px, (float)W));
        i = min(max(i, 0), H - 1);
        j = min(max(j, 0), W - 1);
        const float ry = lte_rel(cy, lte_axpy(a.fy0, a.fys, (float)i), (float)H), rx = lte_rel(cx, lte_axpy(a.fx0, a.fxs, (float)j), (float)W);
        m_pix[tid] = i * W + j;
        m_ry[tid] = ry;
        m_rx[tid] = rx;
        m_area[tid] = hat_add_rn(fabsf(ry * rx), 1e-9f);
        m_ch[tid] = ky * (float)H;
        m_cw[tid] = kx * (float)W;
        if (s == 0) {
            m_cy[q] = cy;
            m_cx[q] = cx;
        }
    }
    __syncthreads();

    // ---- basis: thread = (frequencies 2 k2, 2 k2 + 1; every fourth row)                                        lte.py:79-87
    {
        const int k2 = tid & 63;
        const f32x4 ph = *reinterpret_cast<const f32x4*>(a.phase + 4 * k2);   // Wp[2 k2][0..1], Wp[2 k2 + 1][0..1]
        for (int r = wave; r < LTE_ROWS; r += 4) {
            const int64_t pix = m_pix[r];
            const f32x4 fr = *reinterpret_cast<const f32x4*>(a.freq + pix * a.ldf + 4 * k2);
            const f32x2 cc = *reinterpret_cast<const f32x2*>(a.coef + pix * a.ldc + 2 * k2);
            const f32x2 cs = *reinterpret_cast<const f32x2*>(a.coef + pix * a.ldc + LTE_HID / 2 + 2 * k2);
            const float ry = m_ry[r], rx = m_rx[r], ch = m_ch[r], cw = m_cw[r];
            const float f0 = (fr[0] * ry + fr[1] * rx) + (ph[0] * ch + ph[1] * cw);
            const float f1 = (fr[2] * ry + fr[3] * rx) + (ph[2] * ch + ph[3] * cw);
            float s0, c0, s1, c1;
            lte_sincospi<T>(f0, s0, c0);
            lte_sincospi<T>(f1, s1, c1);
            lte_store2<T>(act + r * LD + 2 * k2, cc[0] * c0, cc[1] * c1);
            lte_store2<T>(act + r * LD + LTE_HID / 2 + 2 * k2, cs[0] * s0, cs[1] * s1);
        }
    }
    __syncthreads();

    // ---- the three 256 x 256 layers; each output replaces its input once every wave has read it               mlp.py:20-23
    f32x4 acc[4][8];
#pragma unroll 1
    for (int l = 0; l < 2; ++l) {
        lte_layer<T>(reinterpret_cast<const T*>(a.w[l]), act, wave, lane, acc);
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int ch = 64 * wave + 16 * tt + 4 * g;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(a.b[l] + ch);
#pragma unroll
            for (int pt = 0; pt < 8; ++pt) {
                f32x4 v = acc[tt][pt] + bias;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                Vec4<T>::store(act + (16 * pt + l15) * LD + ch, v);
            }
        }
        __syncthreads();
    }
    lte_layer<T>(reinterpret_cast<const T*>(a.w[2]), act, wave, lane, acc);

    // ---- the last layer (256 -> 3) from the fp32 accumulators: this wave's 64 channels, summed over the lane groups, then the waves
    {
        float p[8][3];
#pragma unroll
        for (int pt = 0; pt < 8; ++pt) p[pt][0] = p[pt][1] = p[pt][2] = 0.f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int ch = 64 * wave + 16 * tt + 4 * g;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(a.b[2] + ch);
            f32x4 w4[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) w4[c] = *reinterpret_cast<const f32x4*>(a.w4 + c * LTE_HID + ch);
#pragma unroll
            for (int pt = 0; pt < 8; ++pt) {
                f32x4 v = acc[tt][pt] + bias;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
#pragma unroll
                for (int c = 0; c < 3; ++c) p[pt][c] += w4[c][0] * v[0] + w4[c][1] * v[1] + w4[c][2] * v[2] + w4[c][3] * v[3];
            }
        }
#pragma unroll
        for (int pt = 0; pt < 8; ++pt)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = p[pt][c];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (g == 0) part[(wave * LTE_ROWS + 16 * pt + l15) * 3 + c] = v;
            }
    }
    __syncthreads();
    if (tid < LTE_ROWS) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            part[tid * 3 + c] = a.b4[c] + ((part[tid * 3 + c] + part[(LTE_ROWS + tid) * 3 + c]) +
                                           (part[(2 * LTE_ROWS + tid) * 3 + c] + part[(3 * LTE_ROWS + tid) * 3 + c]));
    }
    __syncthreads();

    // ---- the area-weighted sum with the diagonal swap, plus the bilinear base image (border padding)         lte.py:95-104
    if constexpr (std::is_same<Sink, LtePlanes>::value) {
        if (tid < LTE_TQ) {
            const int q = tid;
            bool valid;
            int64_t o0, ostride;
            if (grid) {
                const int oy = ty0 + q / LTE_TX, ox = tx0 + q % LTE_TX;
                valid = oy < a.gh && ox < a.gw;
                o0 = (int64_t)oy * a.gw + ox;
                ostride = (int64_t)a.gh * a.gw;
            } else {
                valid = q0 + q < a.Q;
                o0 = 3 * (q0 + q);
                ostride = 1;
            }
            if (valid) {
                const float a0 = m_area[q], a1 = m_area[LTE_TQ + q], a2 = m_area[2 * LTE_TQ + q], a3 = m_area[3 * LTE_TQ + q];
                const float tot = ((a0 + a1) + a2) + a3;
                const float w0 = a3 / tot, w1 = a2 / tot, w2 = a1 / tot, w3 = a0 / tot;
                const float cy = m_cy[q], cx = m_cx[q];
                float iy = fminf(fmaxf(lte_unnormalize(cy, (float)H), 0.f), (float)(H - 1));
                float ix = fminf(fmaxf(lte_unnormalize(cx, (float)W), 0.f), (float)(W - 1));
                const float fy = floorf(iy), fx = floorf(ix);
                const int y0 = min(max((int)fy, 0), H - 1), x0 = min(max((int)fx, 0), W - 1);
                const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
                const float ty = iy - fy, tx = ix - fx;
                const float wnw = (1.f - tx) * (1.f - ty), wne = tx * (1.f - ty), wsw = (1.f - tx) * ty, wse = tx * ty;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* pl = a.inp + (int64_t)c * H * W;
                    const float base = pl[(int64_t)y0 * W + x0] * wnw + pl[(int64_t)y0 * W + x1] * wne + pl[(int64_t)y1 * W + x0] * wsw +
                                       pl[(int64_t)y1 * W + x1] * wse;
                    float v = part[q * 3 + c] * w0 + part[(LTE_TQ + q) * 3 + c] * w1 + part[(2 * LTE_TQ + q) * 3 + c] * w2 +
                              part[(3 * LTE_TQ + q) * 3 + c] * w3;
                    v += base;
                    a.out[o0 + c * ostride] = v * a.out_a + a.out_b;
                }
            }
        }
    } else {
        // grid mode only.  The whole first wave enters: the YCbCr sink exchanges values between lanes, so no lane may be missing
        // from it; lanes 32 .. 63 and lanes past gh / gw hold zeros.
        if (wave == 0) {
            const int q = lane & (LTE_TQ - 1);
            const int oy = ty0 + q / LTE_TX, ox = tx0 + q % LTE_TX;
            const bool valid = lane < LTE_TQ && oy < a.gh && ox < a.gw;
            float rgb[3] = {0.f, 0.f, 0.f};
            if (valid) lte_pixel(a, q, m_area, m_cy, m_cx, part, rgb);
            sink.store(rgb, valid, oy, ox);
        }
    }
}

template <typename T, typename Sink> int lte_launch(const LteArgs& a, const Sink& sink, int64_t tiles, hipStream_t s) {
    constexpr size_t lds = LteLds<T>::BYTES;
    auto kern = lte_query_kernel<T, Sink>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    HAT_LAUNCH(kern, dim3((unsigned)tiles), dim3(LTE_THREADS), lds, s, a, sink);
    return hat_check_launch();
}

bool aligned(const void* p, uintptr_t al) { return reinterpret_cast<uintptr_t>(p) % al == 0; }

// What every entry checks and fills, from the arguments alone; `out`: where the result goes first (it must not be inp).  Grid mode
// when coord is null.  Returns 0 or HAT_EINVAL.
int lte_args(LteArgs& a, int64_t& tiles, const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
             const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3, const float* b3,
             const float* w4, const float* b4, const float* coord, const float* cell, int64_t Q, int32_t gh, int32_t gw, float cell_y,
             float cell_x, float out_a, float out_b, const void* out, int32_t dtype) {
    if (!coef || !freq || !inp || !phase || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !out) return HAT_EINVAL;
    if (dtype != HAT_F32 && dtype != HAT_BF16) return HAT_EINVAL;
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff) return HAT_EINVAL;
    if (ldc < LTE_HID || ldc % 4 || ldf < LTE_HID || ldf % 4) return HAT_EINVAL;
    if (!aligned(coef, 16) || !aligned(freq, 16) || !aligned(phase, 16) || !aligned(w1, 16) || !aligned(w2, 16) || !aligned(w3, 16) ||
        !aligned(b1, 16) || !aligned(b2, 16) || !aligned(b3, 16) || !aligned(w4, 16) || !aligned(b4, 4) || !aligned(inp, 4))
        return HAT_EINVAL;
    if ((coord == nullptr) != (cell == nullptr)) return HAT_EINVAL;
    a = LteArgs{};
    if (coord) {
        if (Q < 1 || !aligned(coord, 4) || !aligned(cell, 4)) return HAT_EINVAL;
        tiles = (Q + LTE_TQ - 1) / LTE_TQ;
    } else {
        if (gh < 1 || gw < 1 || (int64_t)gh * gw > 0x7fffffff) return HAT_EINVAL;
        a.tiles_x = (gw + LTE_TX - 1) / LTE_TX;
        tiles = (int64_t)((gh + LTE_TY - 1) / LTE_TY) * a.tiles_x;
        Q = (int64_t)gh * gw;
        // make_coord (esc_arb/utils.py:105-120): seq = (v0 + r) + (2 r) * arange(n).float(), r = 1 / n in double
        a.gy0 = (float)(-1.0 + 1.0 / gh), a.gys = (float)(2.0 / gh), a.gx0 = (float)(-1.0 + 1.0 / gw), a.gxs = (float)(2.0 / gw);
    }
    if (tiles > 0x7fffffff) return HAT_EINVAL;
    if (out == reinterpret_cast<const void*>(inp)) return HAT_EINVAL;
    a.coef = coef, a.freq = freq, a.inp = inp, a.phase = phase;
    a.w[0] = w1, a.w[1] = w2, a.w[2] = w3, a.b[0] = b1, a.b[1] = b2, a.b[2] = b3, a.w4 = w4, a.b4 = b4;
    a.coord = coord, a.cell = cell, a.Q = Q;
    a.H = H, a.W = W, a.ldc = ldc, a.ldf = ldf, a.gh = gh, a.gw = gw;
    a.cell_y = cell_y, a.cell_x = cell_x;
    a.fy0 = (float)(-1.0 + 1.0 / H), a.fys = (float)(2.0 / H), a.fx0 = (float)(-1.0 + 1.0 / W), a.fxs = (float)(2.0 / W);
    for (int v = 0; v < 2; ++v) {
        a.sy[v] = (float)((2 * v - 1) * (2.0 / H / 2) + 1e-6);
        a.sx[v] = (float)((2 * v - 1) * (2.0 / W / 2) + 1e-6);
    }
    a.out_a = out_a, a.out_b = out_b;
    return 0;
}

// the bytes [p, p + n) and the input planes share a byte
bool overlaps_inp(const void* p, int64_t n, const float* inp, int32_t H, int32_t W) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), ilo = reinterpret_cast<uintptr_t>(inp);
    return lo < ilo + (uintptr_t)12 * H * W && ilo < lo + (uintptr_t)n;
}

template <typename Sink> int lte_launch_dtype(const LteArgs& a, const Sink& sink, int64_t tiles, int32_t dtype, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return dtype == HAT_BF16 ? lte_launch<bf16_t>(a, sink, tiles, s) : lte_launch<float>(a, sink, tiles, s);
}

}  // namespace

extern "C" int hat_lte_query(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                             const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                             const float* b3, const float* w4, const float* b4, const float* coord, const float* cell, int64_t Q,
                             int32_t gh, int32_t gw, float cell_y, float cell_x, float out_a, float out_b, float* out, int32_t dtype,
                             void* stream) {
    LteArgs a;
    int64_t tiles;
    if (!aligned(out, 4)) return HAT_EINVAL;
    if (int rc = lte_args(a, tiles, coef, freq, ldc, ldf, inp, H, W, phase, w1, b1, w2, b2, w3, b3, w4, b4, coord, cell, Q, gh, gw, cell_y, cell_x,
                          out_a, out_b, out, dtype))
        return rc;
    a.out = out;
    return lte_launch_dtype(a, LtePlanes{}, tiles, dtype, stream);
}

extern "C" int hat_lte_query_u8(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                                const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                                const float* b3, const float* w4, const float* b4, int32_t gh, int32_t gw, float cell_y, float cell_x,
                                float out_a, float out_b, uint8_t* dst, int64_t dst_pitch, int32_t bgr, int32_t dtype, void* stream) {
    LteArgs a;
    int64_t tiles;
    if (int rc = lte_args(a, tiles, coef, freq, ldc, ldf, inp, H, W, phase, w1, b1, w2, b2, w3, b3, w4, b4, nullptr, nullptr, 0, gh, gw, cell_y,
                          cell_x, out_a, out_b, dst, dtype))
        return rc;
    if (dst_pitch < (int64_t)3 * gw || overlaps_inp(dst, dst_pitch * (gh - 1) + (int64_t)3 * gw, inp, H, W)) return HAT_EINVAL;
    return lte_launch_dtype(a, LteU8{dst, (long long)dst_pitch, bgr ? 1 : 0}, tiles, dtype, stream);
}

extern "C" int hat_lte_query_yuv(const float* coef, const float* freq, int32_t ldc, int32_t ldf, const float* inp, int32_t H, int32_t W,
                                 const float* phase, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                                 const float* b3, const float* w4, const float* b4, int32_t gh, int32_t gw, float cell_y, float cell_x,
                                 float out_a, float out_b, const HatYuvSurface* dst, const float* from_rgb12, int32_t dtype, void* stream) {
    LteArgs a;
    int64_t tiles;
    if (!dst || !from_rgb12) return HAT_EINVAL;
    if (int rc = lte_args(a, tiles, coef, freq, ldc, ldf, inp, H, W, phase, w1, b1, w2, b2, w3, b3, w4, b4, nullptr, nullptr, 0, gh, gw, cell_y,
                          cell_x, out_a, out_b, dst->y, dtype))
        return rc;
    if (!hat_yuv_surface_ok(dst, 1, gh, gw)) return HAT_EINVAL;
    const int64_t bps = dst->depth == 8 ? 1 : 2;
    if (overlaps_inp(dst->y, dst->y_pitch * (gh - 1) + bps * gw, inp, H, W)) return HAT_EINVAL;
    if (dst->cb) {
        const int64_t ch = gh >> dst->sub_y, crow = (int64_t)dst->c_step * ((gw >> dst->sub_x) - 1) + bps;
        if (overlaps_inp(dst->cb, dst->c_pitch * (ch - 1) + crow, inp, H, W) || overlaps_inp(dst->cr, dst->c_pitch * (ch - 1) + crow, inp, H, W))
            return HAT_EINVAL;
    }
    return yuv_dispatch(*dst, [&](auto L, auto q) {
        using S = typename decltype(L)::sample_t;
        return lte_launch_dtype(a, LteYuv<S, L.sx, L.sy, L.grey>{yuv_dst<S>(*dst), load_csc(from_rgb12), q}, tiles, dtype, stream);
    });
}
