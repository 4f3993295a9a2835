// hat_attn.hip — overlapping cross-attention (OCAB) core on gfx950.   Contract: include/hat_mi355x.h
// (hat_ocab_attention); reference: hat/archs/hat_arch.py:353-388.
//
// One workgroup (4 waves) per (window, head).  K (nk x d, zero padded to 32 channels) and V
// (transposed: 32 x nk) of the (wse x wse) key window live in LDS, out-of-image keys are exact
// zeros (the reference unfolds AFTER the biased projection with zero padding and does not mask).
// Each wave owns 16-query tiles: S^T = K.Q^T via MFMA 16x16 (A = keys, B = queries) so one lane
// holds, for ONE query, 4 keys of every key tile; softmax statistics are per-lane loops plus two
// cross-lane shuffles; P^T feeds the second MFMA (O^T = V^T.P^T) straight from the accumulator
// registers — the contraction index (key) ordering inside a 32-wide k-step is permuted
// identically for both operands, so no LDS round trip or lane movement is needed for P.
#include <type_traits>

#include "hat_common.h"

namespace {

template <typename T> struct alignas(4 * sizeof(T)) Q4 { T v[4]; };  // 4 consecutive elements, one LDS read

template <typename T> __device__ __forceinline__ float exp_t(float x);
template <> __device__ __forceinline__ float exp_t<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ float exp_t<bf16_t>(float x) { return __expf(x); }

// The LDS image of `nkeys` keys of one head: K [nkeys][ldk] (channels d..dk8 are zeros), V^T [dv][ldv] and, 16-byte aligned
// behind them at byte `tab`, the head's (Mr x Mr) bias table.  The kernels carve their LDS up with it and launch_attn sizes
// the launch with it, so the two cannot drift apart.
struct AttnLds { int dk8, dv, ldk, ldv; size_t tab, bytes; };
__host__ __device__ constexpr AttnLds attn_lds(int nkeys, int d, int Mr, int es) {
    const int dk8 = (d + 7) & ~7;                      // K channels kept in LDS (zero padded d..dk8)
    const int dv = (d + 1) & ~1;                        // V^T rows kept in LDS
    const int ldk = lds_row_elems(dk8, es), ldv = lds_row_elems(nkeys, es);
    const size_t tab = (((size_t)nkeys * ldk + (size_t)dv * ldv) * es + 15) / 16 * 16;
    return {dk8, dv, ldk, ldv, tab, tab + (size_t)Mr * Mr * 4};
}

// What ocab_attn_kernel and ocab_attn_stream_kernel share: one workgroup's view of its (window, head) and every step of the
// attention on it.  The two kernels are two loop orders around these steps; the tuned
// ocab_attn_fast_kernel below shares nothing with them.
// SELF / ODD: see ocab_attn_kernel.
template <typename T>
struct Attn {
    using M = MT<T>;
    struct Query { typename M::frag_t qf; int qy, qx, rid; size_t qpix; };   // one query tile: this lane's query c16 of it
    struct Softmax {                                                         // online-softmax state of one query tile
        f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        float mrun = -3.0e38f, l = 0.f;   // l: per-lane partial; reduced across the 4 lane groups in finish()
        int kh = 0, kw = 0;               // !ODD: key row / column of the lane's 4 keys of the next key tile
    };
    const T* q; const T* kv; T* out;
    const int H, W, C, ws, wse, ldq, ldkv, ldo, shift, pad, d, Mr;
    const AttnLds L;
    T* Ks; T* Vt; float* tab;
    const int tid, g, c16, wave, wx, wy, b, h;
    const size_t img;
    const float* kbw;   // HATX key bias / prune mask of this window (hat_ocab_keybias): nkb floats, -inf = pruned key

    // nkeys: keys resident in LDS at a time; nkb: keys of a window's kb row (the whole padded key window)
    __device__ __forceinline__ Attn(char* smem, int nkeys, int nkb, const T* q, const T* kv, T* out, const float* kb, int H, int W,
                                    int C, int heads, int ws, int wse, int ldq, int ldkv, int ldo, int shift, int pad)
        : q(q), kv(kv), out(out), H(H), W(W), C(C), ws(ws), wse(wse), ldq(ldq), ldkv(ldkv), ldo(ldo), shift(shift), pad(pad),
          d(C / heads), Mr(ws + wse - 1), L(attn_lds(nkeys, d, Mr, sizeof(T))), Ks(reinterpret_cast<T*>(smem)),
          Vt(Ks + (size_t)nkeys * L.ldk), tab(reinterpret_cast<float*>(smem + L.tab)), tid(threadIdx.x), g((tid & 63) >> 4),
          c16(tid & 15), wave(tid >> 6), wx(blockIdx.x), wy(blockIdx.y), b(blockIdx.z / heads), h(blockIdx.z - b * heads),
          img((size_t)b * H * W), kbw(kb ? kb + (((size_t)b * gridDim.y + wy) * gridDim.x + wx) * nkb : nullptr) {}

    __device__ __forceinline__ int band(int v, int n) const { return v < n - ws ? 0 : (v < n - shift ? 1 : 2); }   // of the shift mask

    __device__ __forceinline__ void load_table(const float* __restrict__ bias_rot) const {
        for (int i = tid; i < Mr * Mr; i += 256) tab[i] = bias_rot[(size_t)h * Mr * Mr + i];
    }

    // ---- stage keys [key0, key0 + n) as K [key][32] and V^T [32][key], LDS rows / columns 0 .. n; 2 channels per work item
    template <bool SELF, bool ODD>
    __device__ __forceinline__ void stage(int key0, int n) const {
        const int cpk = L.dk8 / 2;  // channel pairs per key
        for (int i = tid; i < n * cpk; i += 256) {
            const int kl = i / cpk, c = (i - kl * cpk) * 2, key = key0 + kl;
            const int kh = key / wse, kw = key - kh * wse;
            int y = wy * ws - pad + kh, x = wx * ws - pad + kw;
            if (SELF) {
                y += shift; if (y >= H) y -= H;
                x += shift; if (x >= W) x -= W;
            }
            T k0 = to_T<T>(0.f), k1 = k0, v0 = k0, v1 = k0;
            if (c < d && (!ODD || key < wse * wse) && y >= 0 && y < H && x >= 0 && x < W) {
                const T* p = kv + (img + (size_t)y * W + x) * ldkv + h * d + c;
                k0 = p[0]; k1 = p[1];
                v0 = p[C]; v1 = p[C + 1];
            }
            Ks[kl * L.ldk + c] = k0; Ks[kl * L.ldk + c + 1] = k1;
            if (c < L.dv) { Vt[c * L.ldv + kl] = v0; Vt[(c + 1) * L.ldv + kl] = v1; }
        }
    }

    // ---- Q fragment (B operand) of query tile qt: this lane's query, channels 8g..8g+7
    template <bool SELF>
    __device__ __forceinline__ Query load_query(int qt) const {
        Query r;
        const int qi = qt * 16 + c16;
        r.qy = qi / ws; r.qx = qi - r.qy * ws;
        int qyo = wy * ws + r.qy, qxo = wx * ws + r.qx;   // position on the (shifted) frame -> pixel of the map
        r.rid = SELF ? 3 * band(qyo, H) + band(qxo, W) : 0;
        if (SELF) {
            qyo += shift; if (qyo >= H) qyo -= H;
            qxo += shift; if (qxo >= W) qxo -= W;
        }
        r.qpix = img + (size_t)qyo * W + qxo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 8 * g + j;
            r.qf[j] = c < d ? q[r.qpix * ldq + h * d + c] : to_T<T>(0.f);
        }
        return r;
    }

    // The chunk step — S^T tiles, softmax update, O^T update for KCH key tiles — is three calls, and the loops over the
    // key tiles stay in the kernels: a helper that held them would be unrolled on its own before it is inlined, the K / V
    // reads of the stream kernel's four query tiles would then be merged and held in registers, and that kernel spills.

    // ---- S^T tile of the key tile at LDS tile kl: s[r] = S[key = 16 kl + 4g + r][query c16]
    __device__ __forceinline__ f32x4 qk(const Query& qr, int kl) const {
        // channel groups beyond dk8 are clamped: they meet a zero Q fragment, so contribute 0
        const typename M::frag_t kf = M::load(Ks + (kl * 16 + c16) * L.ldk + (8 * g < L.dk8 ? 8 * g : L.dk8 - 8));
        return M::mma(kf, qr.qf, f32x4{0.f, 0.f, 0.f, 0.f});
    }

    // ---- one online-softmax step over the S^T tiles of key tiles kt0 .. kt0 + KCH of the window: s becomes P^T (O is only
    //      d <= 32 wide, so the rescale is 8 registers; this keeps the live S tile set at KCH*4 registers)
    template <int KCH, bool SELF, bool ODD>
    __device__ __forceinline__ void softmax(f32x4 (&s)[KCH], const Query& qr, Softmax& st, int kt0) const {
        if (kbw != nullptr) {   // hatx_arch.py:421-449: + focus bias per key; a pruned key's logit is REPLACED by -1e4
#pragma unroll
            for (int t = 0; t < KCH; ++t) {
                const f32x4 k4 = *reinterpret_cast<const f32x4*>(kbw + (kt0 + t) * 16 + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = k4[r] == -INFINITY ? -1.0e4f : s[t][r] + k4[r];
            }
        }
        float mx = -3.0e38f;
#pragma unroll
        for (int t = 0; t < KCH; ++t) {
            const float* tb = tab + (st.kh - qr.qy + ws - 1) * Mr + (st.kw - qr.qx + ws - 1);
            // the lane's 4 keys share a mask band: shift % 4 == 0 and kw % 4 == 0
            const float madd = (SELF && shift > 0 && 3 * band(wy * ws + st.kh, H) + band(wx * ws + st.kw, W) != qr.rid) ? -100.0f : 0.0f;
            if constexpr (ODD) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = (kt0 + t) * 16 + 4 * g + r;
                    const int khr = key / wse, kwr = key - khr * wse;
                    const int ti = min((khr - qr.qy + ws - 1) * Mr + (kwr - qr.qx + ws - 1), Mr * Mr - 1);
                    s[t][r] = key < wse * wse ? s[t][r] + tab[ti] : -3.0e38f;
                    mx = fmaxf(mx, s[t][r]);
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] += tb[r];
                if (SELF) s[t][r] += madd;
                mx = fmaxf(mx, s[t][r]);
            }
            st.kw += 16;
            while (st.kw >= wse) { st.kw -= wse; ++st.kh; }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mnew = fmaxf(st.mrun, mx);
        const float alpha = exp_t<T>(st.mrun - mnew);
        st.mrun = mnew;
        float lsum = 0.f;
#pragma unroll
        for (int t = 0; t < KCH; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp_t<T>(s[t][r] - mnew);
                s[t][r] = p;
                lsum += p;
            }
        }
        st.l = st.l * alpha + lsum;
        st.o[0] *= alpha;
        st.o[1] *= alpha;
    }

    // ---- O^T += V^T . P^T for the chunk's key tiles 2 kk and (but for the last of an odd KCH) 2 kk + 1, which sit in LDS from key
    //      tile kl0 on: k-slot (g, j) = key 32 kk + 4g + j (j<4) | 32 kk + 16 + 4g + (j-4)
    template <int KCH>
    __device__ __forceinline__ void pv(const f32x4 (&s)[KCH], int kk, int kl0, Softmax& st) const {
        const bool has_b = (2 * kk + 1 < KCH);
        const int kb = has_b ? 2 * kk + 1 : 2 * kk;
        typename M::frag_t pf;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pf[j] = to_T<T>(s[2 * kk][j]);
            pf[j + 4] = has_b ? to_T<T>(s[kb][j]) : to_T<T>(0.f);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            // rows >= d are clamped: their outputs are never stored
            const int vrow = (ct * 16 + c16 < L.dv) ? ct * 16 + c16 : L.dv - 1;
            const T* vr = Vt + (size_t)vrow * L.ldv + (kl0 + 2 * kk) * 16 + 4 * g;
            const Q4<T> va = *reinterpret_cast<const Q4<T>*>(vr);
            const Q4<T> vb = *reinterpret_cast<const Q4<T>*>(vr + (has_b ? 16 : 0));
            typename M::frag_t vf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vf[j] = va.v[j];
                vf[j + 4] = has_b ? vb.v[j] : to_T<T>(0.f);
            }
            st.o[ct] = M::mma(vf, pf, st.o[ct]);
        }
    }

    // ---- store: lane holds channels ct*16 + 4g + r of query c16
    __device__ __forceinline__ void finish(const Query& qr, const Softmax& st) const {
        float l = st.l;
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = ct * 16 + 4 * g + r;
                if (c < d) out[qr.qpix * ldo + h * d + c] = to_T<T>(st.o[ct][r] * inv);
            }
        }
    }
};

// One workgroup (4 waves) per (window, head), the whole key window resident in LDS; every wave finishes one query tile after
// the other.
// SELF = true turns the same kernel into (shifted-)window self-attention, (S)W-MSA of swinir_arch.py:140-172, 291-317:
// the key window is the query window (wse == ws), window coordinates live on the cyclically shifted frame (pixel
// (Y, X) of the shifted frame is pixel ((Y + shift) % H, (X + shift) % W) of the map, so the two torch.roll calls become
// addressing), and pairs whose positions fall in different bands of the shift mask (:262-280) get -100 added after the
// bias, exactly as the reference adds its mask tensor.
// ODD: wse % 4 != 0 (HATX: window 16, overlap 0.6 -> 25 x 25 keys).  The key window is stored as NKT * 16 >= wse * wse keys: the
// keys past wse * wse are dead (zero K / V, logit -3e38 so that they vanish from the softmax), and a lane's four keys of a
// tile may sit in two key rows, so each looks up its own bias entry.
template <typename T, int NKT, int KCH, bool SELF, bool ODD = false>
__global__ __launch_bounds__(256) void ocab_attn_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                        const float* __restrict__ bias_rot, T* __restrict__ out, int H, int W,
                                                        int C, int heads, int ws, int wse, int ldq, int ldkv, int ldo,
                                                        int shift, const float* __restrict__ kb, int pad) {
    constexpr int NK = NKT * 16;
    static_assert(NKT % KCH == 0, "key tiles must split evenly into chunks");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Attn<T> a(smem, NK, NK, q, kv, out, kb, H, W, C, heads, ws, wse, ldq, ldkv, ldo, shift, pad);
    a.load_table(bias_rot);
    a.template stage<SELF, ODD>(0, NK);
    __syncthreads();

    const int nqt = (ws * ws) / 16;
    for (int qt = a.wave; qt < nqt; qt += 4) {
        const typename Attn<T>::Query qr = a.template load_query<SELF>(qt);
        typename Attn<T>::Softmax st;
        st.kh = (4 * a.g) / wse; st.kw = 4 * a.g - st.kh * wse;  // the lane's 4 keys of a tile share one key row (wse % 4 == 0)
#pragma unroll 1
        for (int ch = 0; ch < NKT / KCH; ++ch) {
            const int kt0 = ch * KCH;
            f32x4 s[KCH];
#pragma unroll
            for (int t = 0; t < KCH; ++t) s[t] = a.qk(qr, kt0 + t);
            a.template softmax<KCH, SELF, ODD>(s, qr, st, kt0);
#pragma unroll
            for (int kk = 0; kk < (KCH + 1) / 2; ++kk) a.template pv<KCH>(s, kk, kt0, st);
        }
        a.finish(qr, st);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Key-STREAMING form of the generic kernel, for key windows whose K / V image does not fit in LDS — the exact-fp32 path at
// the fork's live HATX shape (hatx_arch.py:289-465 with overlap_ratio 0.6: 25 x 25 keys in 40 tiles x 30-channel heads in
// fp32 = 169 KB).  The online softmax already consumed the keys in chunks of KCH tiles; here only ONE chunk of K and V^T is
// resident (KCH = 10: 43 KB), staged by the whole workgroup between two barriers, and every wave carries the softmax state
// (O, running max, partial denominator) of ALL its NQW query tiles across the chunks instead of finishing one query tile
// after the other.  The steps are ocab_attn_kernel's own (Attn<T>, with its ODD handling: dead keys past wse^2, per-key bias
// lookup), on the key chunks in the same order.  Instantiated only where a window can fail to fit (attn_may_stream).
// ---------------------------------------------------------------------------------------------------------
template <typename T, int NKT, int KCH, int NQW>
__global__ __launch_bounds__(256) void ocab_attn_stream_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                               const float* __restrict__ bias_rot, T* __restrict__ out, int H, int W,
                                                               int C, int heads, int ws, int wse, int ldq, int ldkv, int ldo,
                                                               const float* __restrict__ kb, int pad) {
    constexpr int NK = NKT * 16, CK = KCH * 16;
    static_assert(NKT % KCH == 0, "key tiles must split evenly into chunks");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Attn<T> a(smem, CK, NK, q, kv, out, kb, H, W, C, heads, ws, wse, ldq, ldkv, ldo, 0, pad);
    a.load_table(bias_rot);
    typename Attn<T>::Query qr[NQW];
    typename Attn<T>::Softmax st[NQW];
#pragma unroll
    for (int i = 0; i < NQW; ++i) qr[i] = a.template load_query<false>(a.wave + 4 * i);
#pragma unroll 1
    for (int ch = 0; ch < NKT / KCH; ++ch) {
        __syncthreads();   // every wave is done with the previous chunk (first pass: the bias table is complete)
        a.template stage<false, true>(ch * CK, CK);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NQW; ++i) {
            f32x4 s[KCH];
#pragma unroll
            for (int t = 0; t < KCH; ++t) s[t] = a.qk(qr[i], t);
            a.template softmax<KCH, false, true>(s, qr[i], st[i], ch * KCH);
#pragma unroll
            for (int kk = 0; kk < (KCH + 1) / 2; ++kk) a.template pv<KCH>(s, kk, 0, st[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NQW; ++i) a.finish(qr[i], st[i]);
}

// ---------------------------------------------------------------------------------------------------------
// Fast path: bf16, 16x16 query windows, 24x24 key windows, head_dim 24 (HAT-S and every C = 144 model).
// Differences from the generic kernel above, all aimed at the VALU (softmax) and LDS-store bottlenecks:
//   * K and V are staged with 16-byte pieces, V row-major [key][32] (no 2-byte transposing stores); the A
//     operand V^T of the second MFMA is read with ds_read_b64_tr_b16 (hardware transpose);
//   * V carries a constant-1 column at channel 24, so the softmax denominator is output row 24 of the same
//     MFMA (it is rescaled with O for free in the online-softmax update): no VALU row sums;
//   * the relative-position bias enters as the C operand of the S MFMA: no VALU bias adds;
//   * p = exp2(fma(s, log2e, -m*log2e)): one FMA + one exp per score.
// ---------------------------------------------------------------------------------------------------------
// v_max3_f32 without the per-input canonicalising v_max the compiler adds for fmaxf (scores are never NaN-signalling)
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// max(|a|, |b|, |c|) in one instruction (VOP3 abs modifiers)
__device__ __forceinline__ float max3_abs(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// D = 24 (C = 144) or 30 (C = 180, six heads): D = 30 pads K / Q to 32 channels (K rows of 4 XOR-swizzled slots), stages
// and stores with 4-byte accesses (a head's 60-byte slice is only 4-byte aligned) and keeps the ones column at V[30].
// WSE = 24, SELF = false: OCAB (zero-padded 24 x 24 key window around the query window).  WSE = 16, SELF = true: (shifted-)
// window self-attention for hat_window_attention — the key window is the query window, all coordinates live on the frame
// shifted cyclically by `shift` (so every key is a real pixel), and in the last window row / column the -100 of the
// shift mask is added to the scores of pairs in different mask bands.
// NTH: threads per workgroup.  512 (the OCAB of the C = 144 models) = eight waves with two query rows each and key chunks of 6
// tiles (half the score registers: 80 VGPRs): the K / V image of a 24 x 24 key window (64.5 KB) limits a CU to two workgroups,
// and sixteen waves instead of eight hide more of the softmax's latencies (0.995 -> 0.955 ms at 720p; sixteen-wave workgroups
// measured the same as eight).
template <int D, int WSE, bool SELF, int NTH = 256, bool QLOG2 = false>
__global__ __launch_bounds__(NTH, WSE == 24 ? 2 : 4) void ocab_attn_fast_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv,
                                                                const float* __restrict__ bias_rot, bf16_t* __restrict__ out,
                                                                int B, int H, int W, int C, int heads, int ldq, int ldkv,
                                                                int ldo, int shift) {
    using M = MT<bf16_t>;
    using frag_t = M::frag_t;
    constexpr int WS = 16, NK = WSE * WSE, MR = WS + WSE - 1, NKT = NK / 16, KCH = WSE == 24 ? (NTH >= 512 ? 6 : 12) : 8, PAD = (WSE - WS) / 2;
    constexpr int CH_ROWS = KCH * 16 / WSE;  // key rows per chunk
    static_assert(KCH % 2 == 0 && KCH * 16 % WSE == 0, "a chunk is whole key rows and whole pairs of key tiles");
    static_assert(!SELF || WSE == WS, "self-attention windows coincide with the query windows");
    // OFFS (the OCAB of the embed_dim-144 models): the softmax offset rides in the spare k-slots of the QK^T MFMA.  K rows
    // are 32 channels wide with [1.0, 0 ...] in channels 24..31 of EVERY key, the query fragment carries -m (the running
    // offset, a bf16 value, in log2 units) in channel 24, Q and the bias table are pre-multiplied by log2(e): the MFMA
    // delivers s * log2e + bias * log2e - m, and p = exp2 of that with NO per-score FMA, no per-chunk rescale of O and no
    // cross-lane max — while every |score - m| of a chunk stays below 64 (checked with 12 v_max3 |.| and one ballot); a chunk
    // that leaves that range takes the classic path (re-centre, rescale O) and moves m.
    constexpr bool OFFS = QLOG2 && D == 24 && WSE == 24 && !SELF;
    constexpr int KR = (D == 24 && !OFFS) ? 24 : 32;   // K row length in LDS (elements)
    constexpr int ONE = D == 24 ? 24 : 30;  // V column that holds 1.0 (the softmax denominator row of O^T)
    constexpr float LOG2E = 1.4426950408889634f;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);                 // [NK][KR]
    bf16_t* Vs = Ks + NK * KR;                                    // [NK][32]: D channels, 1.0, zeros
    float* tab = reinterpret_cast<float*>(Vs + NK * 32);          // [MR*MR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
    // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  A head reads a 2D-byte slice of every q / k / v
    // row, i.e. part of a cache line that the window's other heads need too: block L -> XCD L % 8, and inside an XCD
    // consecutive blocks are the heads of ONE window, so the lines are fetched from HBM once and hit in that XCD's L2
    // (with the head as the slowest grid index every head re-fetched them: 0.82 -> 0.43 ms for W-MSA, 0.97 -> 0.88 ms for
    // OCAB at 720p; giving each XCD a contiguous range of windows instead of every 8th one measured no better).
    const int nwx = W / WS, nwy = H / WS;
    const int xj = (int)blockIdx.x >> 3;
    const int widx = (xj / heads) * 8 + ((int)blockIdx.x & 7), h = xj % heads;
    if (widx >= B * nwx * nwy) return;   // whole workgroup, before any barrier
    const int b = widx / (nwx * nwy), wrem = widx - b * nwx * nwy;
    const int wy = wrem / nwx, wx = wrem - wy * nwx;
    const size_t img = (size_t)b * H * W;
    // window position (row, col) -> pixel of the map: identity for OCAB queries, cyclic shift for SELF
    auto qpixel = [&](int row, int col) {
        int y = wy * WS + row, x = wx * WS + col;
        if (SELF) {
            y += shift; if (y >= H) y -= H;
            x += shift; if (x >= W) x -= W;
        }
        return img + (size_t)y * W + x;
    };
    // key (kh, kw) of the key window -> clamped pixel and whether it is a real one (SELF: always, after the wrap)
    auto kpixel = [&](int kh, int kw, bool& inb) {
        if (SELF) { inb = true; return qpixel(kh, kw); }
        const int y = wy * WS - PAD + kh, x = wx * WS - PAD + kw;
        inb = y >= 0 && y < H && x >= 0 && x < W;
        return img + (size_t)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1);
    };

    constexpr int NWV = NTH / 64, QPW = 16 / NWV;   // waves, query rows (tiles) per wave
    frag_t qfr[QPW];   // this wave's query tiles: query tile qt = window row qt, lane c16 = window column
    constexpr int NTAB = (MR * MR + NTH - 1) / NTH;
    float tv[NTAB];
#pragma unroll
    for (int it = 0; it < NTAB; ++it) {
        const int i = tid + it * NTH;
        tv[it] = bias_rot[(size_t)h * MR * MR + (i < MR * MR ? i : MR * MR - 1)] * (OFFS ? LOG2E : 1.0f);
    }
    if constexpr (D == 24) {
        // Every global load of the staging phase is issued before the first LDS store (branch-free: out-of-image keys
        // load a clamped pixel and are zeroed by a select), so the phase costs one memory latency, not nine.
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
            const size_t qpix = qpixel(wave + NWV * i, c16);
            qfr[i] = M::load(q + qpix * ldq + h * D + 8 * (g < 3 ? g : 2));
            if (g == 3) qfr[i] = M::zero();
            // (OFFS: q arrives multiplied by head_dim^-1/2 * log2(e) — the factor is folded into the projection's weights
            // before they are rounded, hat_ocab_attention_log2 — so the scores are in log2 units without another rounding)
        }
        constexpr int NIT = (NK * 4 + NTH - 1) / NTH;   // (the last pass is partial with 512 threads: clamped loads, masked stores)
        u32x4 kq[NIT], vq[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = min(tid + it * NTH, NK * 4 - 1);
            const int key = i >> 2, c = i & 3;
            const int kh = key / WSE, kw = key - kh * WSE;
            bool inb;
            const bf16_t* p = kv + kpixel(kh, kw, inb) * ldkv + h * D + 8 * (c < 3 ? c : 2);
            kq[it] = *reinterpret_cast<const u32x4*>(p);
            vq[it] = *reinterpret_cast<const u32x4*>(p + C);
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * NTH;
            const int key = i >> 2, c = i & 3;
            const int kh = key / WSE, kw = key - kh * WSE;
            bool inb;
            (void)kpixel(kh, kw, inb);
            const int vsw = (key >> 1) & 2;  // rows 4..7 of every 8 swap their 32-byte halves: transposed reads stay conflict-free
            const u32x4 zero = {0u, 0u, 0u, 0u};
            // channel 24 = 1.0 for EVERY key (out-of-image keys still count in the softmax denominator)
            const u32x4 vval = c == 3 ? u32x4{0x00003F80u, 0u, 0u, 0u} : (inb ? vq[it] : zero);
            if (NIT * NTH == NK * 4 || i < NK * 4) {
                *reinterpret_cast<u32x4*>(Vs + key * 32 + 8 * (c ^ vsw)) = vval;
                if constexpr (OFFS) {   // 4 slots per row, XOR-swizzled by the row (conflict-free ds_read_b128); slot 3 = [1.0, 0 ...]
                    const u32x4 kval = c == 3 ? u32x4{0x00003F80u, 0u, 0u, 0u} : (inb ? kq[it] : zero);
                    *reinterpret_cast<u32x4*>(Ks + key * KR + 8 * (c ^ ((key >> 1) & 3))) = kval;
                } else if (c < 3) {
                    *reinterpret_cast<u32x4*>(Ks + key * KR + 8 * c) = inb ? kq[it] : zero;
                }
            }
        }
    } else {
        // 4-byte staging: dword dw (two channels) of key `key`; dword 15 is the pad of K and [1.0, 0] of V
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
            const size_t qpix = qpixel(wave + NWV * i, c16);
            const unsigned* qp = reinterpret_cast<const unsigned*>(q + qpix * ldq + h * D) + 4 * g;
            u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = qp[min(4 * g + j, D / 2 - 1) - 4 * g];
            if (g == 3) v[3] = 0u;   // channels 30, 31
            qfr[i] = __builtin_bit_cast(frag_t, v);
        }
        constexpr int BATCH = WSE == 24 ? (NTH == 512 ? 9 : 12) : 8, NPASS = NK * 16 / NTH / BATCH;
        static_assert(NPASS * BATCH * NTH == NK * 16, "staging passes must cover the key window exactly");
        unsigned* Kd = reinterpret_cast<unsigned*>(Ks);
        unsigned* Vd = reinterpret_cast<unsigned*>(Vs);
        for (int ps = 0; ps < NPASS; ++ps) {
            unsigned kq[BATCH], vq[BATCH];
#pragma unroll
            for (int it = 0; it < BATCH; ++it) {
                const int i = tid + (ps * BATCH + it) * NTH;
                const int key = i >> 4, dw = i & 15;
                const int kh = key / WSE, kw = key - kh * WSE;
                bool inb;
                const unsigned* p = reinterpret_cast<const unsigned*>(kv + kpixel(kh, kw, inb) * ldkv + h * D) + min(dw, D / 2 - 1);
                kq[it] = p[0];
                vq[it] = p[C / 2];
            }
#pragma unroll
            for (int it = 0; it < BATCH; ++it) {
                const int i = tid + (ps * BATCH + it) * NTH;
                const int key = i >> 4, dw = i & 15;
                const int kh = key / WSE, kw = key - kh * WSE;
                bool inb;
                (void)kpixel(kh, kw, inb);
                const int slot = dw >> 2, vsw = (key >> 1) & 2, ksw = (key >> 1) & 3;
                Kd[key * 16 + 4 * (slot ^ ksw) + (dw & 3)] = (inb && dw < D / 2) ? kq[it] : 0u;
                Vd[key * 16 + 4 * (slot ^ vsw) + (dw & 3)] = dw == 15 ? 0x00003F80u : (inb ? vq[it] : 0u);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < NTAB; ++it) {
        const int i = tid + it * NTH;
        if (i < MR * MR) tab[i] = tv[it];
    }
    __syncthreads();

    const int trq = c16 >> 2, trp = c16 & 3;  // this lane's address role inside its 16-lane transpose group
    // Bias-table offsets of this lane's 4 keys (rows 4g..4g+3 of key tile t; WSE % 4 == 0 keeps them in one key
    // row) against query column c16 of window row 0.  A chunk of KCH key tiles is exactly 8 key rows and a query
    // tile is exactly one window row, so chunk ch / query tile qt only add the uniform (8 * ch - qt) * MR.
    int toff[KCH];
#pragma unroll
    for (int t = 0; t < KCH; ++t) {
        const int key = t * 16 + 4 * g;
        const int kh = key / WSE, kw = key - kh * WSE;
        toff[t] = (kh + WS - 1) * MR + (kw - c16 + WS - 1);
    }
#pragma unroll
    for (int qi4 = 0; qi4 < QPW; ++qi4) {
        const int qt = wave + NWV * qi4;
        const size_t qpix = qpixel(qt, c16);
        frag_t qf = qfr[qi4];
        // D = 24: lanes g == 3 meet a zero Q fragment and re-read group 2; D = 30: 4 slots per row, XOR-swizzled by the row
        const bf16_t* krow = (D == 24 && !OFFS) ? Ks + c16 * KR + (g < 3 ? 8 * g : 16) : Ks + c16 * KR + 8 * (g ^ ((c16 >> 1) & 3));
        f32x4 o[2];
        // OFFS: every LDS address of the (fully unrolled) chunk loop is a per-lane base plus an immediate; rolled up, 23 of the
        // 76 vector instructions per 12 MFMAs were address additions.  The bias reads (four consecutive floats at a 4-byte-
        // aligned address) get their per-lane bases once per query tile — 8 ch key rows further down the table is an
        // immediate — and are `volatile`: left alone the load/store optimizer pairs them into ds_read2_b32, whose 8-bit
        // offsets do not reach, and re-creates a base register with a v_add for every pair.
        typedef const volatile __attribute__((address_space(3))) float* lds_vf_p;
        lds_vf_p tq[KCH];
        if constexpr (OFFS) {
#pragma unroll
            for (int t = 0; t < KCH; ++t) tq[t] = (lds_vf_p)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(tab + toff[t] - qt * MR);
        }
        // One pass over the key window.  OFFS has two forms of it:
        //   CHECKED = false (always tried first): the first chunk centres the offset on its row maximum and every later chunk
        //     trusts it — no range check at all (it was 12 v_max3 |.| + a ballot per chunk, a sixth of the loop's VALU time).  A
        //     later score far ABOVE the offset only makes p large (exp2 of up to ~100 is an ordinary float and bf16 has the same
        //     exponent range); what cannot be represented shows in the denominator, and then
        //   CHECKED = true: the pass is repeated with the range check and the re-centring step in every chunk (rare: it takes a
        //     score 2^100 times the first chunk's maximum).
        auto pass = [&](auto checked_tag) {
            constexpr bool CHECKED = decltype(checked_tag)::value;
            float moff = 0.f;   // OFFS: the offset currently riding in the query fragment's channel 24 (log2 units, a bf16 value)
            if constexpr (OFFS) { if (g == 3) qf[0] = (bf16_t)0.f; }
            o[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            o[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            float mrun = -3.0e38f;
            constexpr int UNR = (OFFS && !CHECKED) ? NKT / KCH : 1;
#pragma unroll UNR
            for (int ch = 0; ch < NKT / KCH; ++ch) {
                const int kt0 = ch * KCH;
                const float* tbase = tab + (CH_ROWS * ch - qt) * MR;
                f32x4 s[KCH];
#pragma unroll
                for (int t = 0; t < KCH; ++t) {
                    f32x4 bias4;
                    if constexpr (OFFS && !CHECKED) {
                        lds_vf_p tb = tq[t] + CH_ROWS * ch * MR;
                        bias4 = f32x4{tb[0], tb[1], tb[2], tb[3]};
                    } else {
                        const float* tb = tbase + toff[t];
                        bias4 = f32x4{tb[0], tb[1], tb[2], tb[3]};
                    }
                    const frag_t kf = M::load(krow + (kt0 + t) * 16 * KR);
                    s[t] = M::mma(kf, qf, bias4);
                }
                if constexpr (SELF) {
                    // Shift mask (swinir_arch.py:262-280): bands [0, n-ws), [n-ws, n-shift), [n-shift, n) of the shifted frame,
                    // so only the last window row / column mixes bands.  Key tile t is key row kt0 + t, the query tile is
                    // query row qt (both wave-uniform); the lane's 4 key columns 4g.. share a band (shift % 4 == 0).
                    const bool lastr = wy == nwy - 1, lastc = wx == nwx - 1;
                    if (shift > 0 && (lastr || lastc)) {
                        const float xm = (lastc && ((4 * g >= WS - shift) != (c16 >= WS - shift))) ? -100.0f : 0.0f;
#pragma unroll
                        for (int t = 0; t < KCH; ++t) {
                            const bool ydiff = lastr && ((kt0 + t >= WS - shift) != (qt >= WS - shift));
                            const float madd = ydiff ? -100.0f : xm;
                            s[t][0] += madd; s[t][1] += madd; s[t][2] += madd; s[t][3] += madd;
                        }
                    }
                }
                float c2 = 0.f;      // exponent offset applied on the VALU (classic path only)
                if constexpr (OFFS) {
                    bool plain = ch > 0;   // (uniform) the offset the MFMA applied is good enough for this chunk
                    if constexpr (CHECKED) {
                        float am = 0.f;
#pragma unroll
                        for (int t = 0; t < KCH; ++t) am = max3_abs(max3_abs(am, s[t][0], s[t][1]), s[t][2], s[t][3]);
                        plain = ch > 0 && __builtin_amdgcn_ballot_w64(am > 64.0f) == 0ull;
                    }
                    // The first chunk always centres on its row maximum (any sign: nothing is accumulated yet, and a row whose every
                    // logit lies far below zero must not underflow as a whole); later chunks (CHECKED) re-centre only UPWARDS, when
                    // a score is more than 2^64 above the offset (a score far below it just contributes nothing).
                    if (!plain) {
                        float mx = -3.0e38f;
#pragma unroll
                        for (int t = 0; t < KCH; ++t) mx = max3_raw(max3_raw(mx, s[t][0], s[t][1]), s[t][2], s[t][3]);
                        mx = fmaxf(mx, __shfl_xor(mx, 16));
                        mx = fmaxf(mx, __shfl_xor(mx, 32));
                        const float mnew = (float)(bf16_t)(moff + (ch == 0 ? mx : fmaxf(mx, 0.f)));   // what channel 24 can hold
                        const float delta = mnew - moff;                           // (exact: both are short; >= 0 after the first chunk)
                        if (ch > 0) {
                            const float alpha = __builtin_amdgcn_exp2f(-delta);    // <= 1
                            o[0] *= alpha;
                            o[1] *= alpha;
                        }
#pragma unroll
                        for (int t = 0; t < KCH; ++t) s[t] -= f32x4{delta, delta, delta, delta};
                        moff = mnew;
                        if (g == 3) qf[0] = (bf16_t)(-moff);
                    }
                } else {
                    float mx = -3.0e38f;
#pragma unroll
                    for (int t = 0; t < KCH; ++t) mx = max3_raw(max3_raw(mx, s[t][0], s[t][1]), s[t][2], s[t][3]);
                    mx = fmaxf(mx, __shfl_xor(mx, 16));
                    mx = fmaxf(mx, __shfl_xor(mx, 32));
                    const float mnew = fmaxf(mrun, mx);
                    const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * LOG2E);  // raw v_exp_f32: underflow flushes to 0
                    mrun = mnew;
                    c2 = -mnew * LOG2E;
                    o[0] *= alpha;
                    o[1] *= alpha;
                }
#pragma unroll
                for (int kk = 0; kk < KCH / 2; ++kk) {
                    frag_t pf;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (OFFS) {
                            pf[j] = (bf16_t)__builtin_amdgcn_exp2f(s[2 * kk][j]);
                            pf[4 + j] = (bf16_t)__builtin_amdgcn_exp2f(s[2 * kk + 1][j]);
                        } else {
                            pf[j] = (bf16_t)__builtin_amdgcn_exp2f(fmaf(s[2 * kk][j], LOG2E, c2));
                            pf[4 + j] = (bf16_t)__builtin_amdgcn_exp2f(fmaf(s[2 * kk + 1][j], LOG2E, c2));
                        }
                    }
                    const int key0 = (kt0 + 2 * kk) * 16 + 4 * g;
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        typedef short s16x4 __attribute__((ext_vector_type(4)));
                        typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_p;
                        const bf16_t* va = Vs + (key0 + trq) * 32 + (ct ^ (g & 1)) * 16 + 4 * trp;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(va + 16 * 32));
                        typedef short s16x8 __attribute__((ext_vector_type(8)));
                        const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        o[ct] = M::mma(__builtin_bit_cast(frag_t, both), pf, o[ct]);
                    }
                }
            }
            // row ONE of O^T is the softmax denominator: register (ONE - 16) % 4 of lane group (ONE - 16) / 4, second tile
            return __shfl(o[1][(ONE - 16) & 3], 16 * ((ONE - 16) >> 2) + c16);
        };
        float l = pass(std::false_type{});
        if constexpr (OFFS) {
            // (the query tile's 16 denominators: all finite and far from the top of the range, or the pass is repeated)
            if (__builtin_amdgcn_ballot_w64(!(l < 1.0e30f)) != 0ull) {
                asm volatile("; repeat the pass with range checks (rare path: keep it a branch)" ::: "memory");
                l = pass(std::true_type{});
            }
        }
        const float inv = 1.0f / l;
        bf16_t* op = out + qpix * ldo + h * D + 4 * g;
        if constexpr (D == 24) {
            Vec4<bf16_t>::store(op, o[0] * inv);
            if (g < 2) Vec4<bf16_t>::store(op + 16, o[1] * inv);
        } else {  // 4-byte stores: the head slice is only 4-byte aligned; channels 28, 29 are the last two
            typedef bf16_t bf2 __attribute__((ext_vector_type(2)));
            const f32x4 a0 = o[0] * inv, a1 = o[1] * inv;
            *reinterpret_cast<bf2*>(op) = bf2{(bf16_t)a0[0], (bf16_t)a0[1]};
            *reinterpret_cast<bf2*>(op + 2) = bf2{(bf16_t)a0[2], (bf16_t)a0[3]};
            *reinterpret_cast<bf2*>(op + 16) = bf2{(bf16_t)a1[0], (bf16_t)a1[1]};
            if (g < 3) *reinterpret_cast<bf2*>(op + 18) = bf2{(bf16_t)a1[2], (bf16_t)a1[3]};
        }
    }
}


// ---------------------------------------------------------------------------------------------------------
// HATX key bias / prune mask (hatx_arch.py:421-449): one workgroup per key window, one thread per key.
//   score = tanh(saliency at the key's pixel)  (0 for the zero-padded keys outside the image: tanh(0)), or ||k||_2 over all
//   channels when there is no focus head; the k_keep keys with the largest score are kept — among EQUAL scores the key with
//   the lower window index (torch.topk leaves that order unspecified: DESIGN.md §7) —, kb = focus score (0 without focus
//   head) for a kept key and -inf for a pruned one.
// ---------------------------------------------------------------------------------------------------------
template <typename T, typename ST = T>
__global__ __launch_bounds__(1024) void keybias_kernel(const ST* __restrict__ sal, int ldsal, const T* __restrict__ kv, int ldkv,
                                                       float* __restrict__ kb, int H, int W, int C, int ws, int wse, int pad, int k_keep) {
    __shared__ float sc[1024];
    const int nk = wse * wse, nkp = (nk + 15) & ~15, key = threadIdx.x;   // rows of nkp floats: the attention kernel's key tiles
    const int wx = blockIdx.x, wy = blockIdx.y, b = blockIdx.z;
    float s = 0.f;
    if (key < nk) {
        const int kh = key / wse, kw = key - kh * wse;
        const int y = wy * ws - pad + kh, x = wx * ws - pad + kw;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t pix = ((size_t)b * H + y) * W + x;
            if (sal != nullptr) {
                s = tanhf(to_f(sal[pix * ldsal]));
            } else {
                float q = 0.f;
                for (int c = 0; c < C; ++c) { const float v = to_f(kv[pix * ldkv + c]); q += v * v; }
                s = sqrtf(q);
            }
        }
    }
    sc[key] = s;
    __syncthreads();
    if (key < nk) {
        bool keep = true;
        if (k_keep < nk) {
            int rank = 0;
            for (int j = 0; j < nk; ++j) rank += (sc[j] > s || (sc[j] == s && j < key)) ? 1 : 0;
            keep = rank < k_keep;
        }
        kb[(((size_t)b * gridDim.y + wy) * gridDim.x + wx) * nkp + key] = keep ? (sal != nullptr ? s : 0.f) : -INFINITY;
    } else if (key < nkp) {   // dead keys of the padded window (odd wse): the attention kernel ignores the value
        kb[(((size_t)b * gridDim.y + wy) * gridDim.x + wx) * nkp + key] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------
// What hat_ocab_attention, hat_ocab_attention_kb and hat_window_attention all refuse, in the order they always tested it;
// `window_ok` holds the entry's own conditions on the windows and runs between the two shared lines.
template <typename F>
int attn_check(bool ptrs, int B, int C, int heads, int ldq, int ldkv, int ldo, F window_ok) {
    if (!ptrs || B < 1 || heads < 1 || C % heads) return HAT_EINVAL;
    if (!window_ok()) return HAT_EINVAL;
    const int d = C / heads;
    if (d > 32 || d % 2 || ldq < C || ldkv < 2 * C || ldo < C) return HAT_EINVAL;
    return 0;
}

// Raise the dynamic-LDS limit where the launch needs more than the default 64 KiB, launch, report.
template <typename K, typename... A>
int attn_launch(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, A... args) {
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    HAT_LAUNCH(kern, grid, dim3(threads), lds, s, args...);
    return hat_check_launch();
}

struct AttnArgs {   // one call of a generic kernel; pad < 0: the ceiling (HATX pads odd overlaps with it, hatx_arch.py:303-305)
    const void* q; const void* kv; const float* bias; void* out;
    int B, H, W, C, heads, ws, wse, ldq, ldkv, ldo;
    hipStream_t s;
    int shift; const float* kb; int pad;
};

// Whether a key window of nkt tiles may have to be streamed: not when its resident image fits in LDS for every call that
// reaches ocab_attn_stream_kernel.  The stream kernel takes ws == 16 only, the entries admit d <= 32 and attn_lds grows
// with d, and nkt tiles hold wse * wse <= 16 nkt keys, which bounds the table.  Where this is false, a call whose image does
// not fit has ws != 16, which the streaming branch refuses with HAT_ELDS as well — so launch_attn returns the same code
// with the stream kernel never instantiated.  True for fp32 with 40 key tiles alone (25 x 25 keys: 92 160 B of K + 82 432 B
// of V^T at d = 32); fp32 with 36 tiles is 163 268 B and bf16 with 40 tiles 109 824 B.
constexpr bool attn_may_stream(int nkt, int es) {
    int wse = 0;
    while ((wse + 1) * (wse + 1) <= 16 * nkt) ++wse;
    return attn_lds(16 * nkt, 32, 16 + wse - 1, es).bytes > HAT_LDS_MAX;
}

template <typename T, int NKT, int KCH, bool SELF, bool ODD>
int launch_attn(const AttnArgs& a) {
    const int pad = a.pad < 0 ? (a.wse - a.ws + 1) / 2 : a.pad;
    const int Mr = a.ws + a.wse - 1, d = a.C / a.heads;
    const dim3 grid(a.W / a.ws, a.H / a.ws, a.B * a.heads);
    const T* q = reinterpret_cast<const T*>(a.q);
    const T* kv = reinterpret_cast<const T*>(a.kv);
    T* out = reinterpret_cast<T*>(a.out);
    const size_t lds = attn_lds(NKT * 16, d, Mr, sizeof(T)).bytes;
    if (lds <= HAT_LDS_MAX)
        return attn_launch(ocab_attn_kernel<T, NKT, KCH, SELF, ODD>, grid, 256, lds, a.s, q, kv, a.bias, out, a.H, a.W, a.C, a.heads, a.ws,
                           a.wse, a.ldq, a.ldkv, a.ldo, a.shift, a.kb, pad);
    // the key window does not fit: stream it through LDS chunk by chunk (instantiated for 16 x 16 query windows)
    if constexpr (!SELF && attn_may_stream(NKT, sizeof(T))) {
        const size_t lds2 = attn_lds(KCH * 16, d, Mr, sizeof(T)).bytes;
        if (a.ws == 16 && lds2 <= HAT_LDS_MAX)
            return attn_launch(ocab_attn_stream_kernel<T, NKT, KCH, 4>, grid, 256, lds2, a.s, q, kv, a.bias, out, a.H, a.W, a.C, a.heads,
                               a.ws, a.wse, a.ldq, a.ldkv, a.ldo, a.kb, pad);
    }
    return HAT_ELDS;
}

// The generic kernels' instantiations by key-window size.  OCAB: 24 / 12 (HAT: window 16 / 8, overlap 0.5), 25 (HATX training
// config: window 16, overlap 0.6; 625 keys in 40 tiles) and 13 (window 8, overlap 0.7: the small model of the goldens).
// SELF: the key window is the query window, 16 or 8.
template <typename T, bool SELF>
int attn_by_window(const AttnArgs& a) {
    if constexpr (SELF) {
        if (a.wse == 16) return launch_attn<T, 16, 8, true, false>(a);
        if (a.wse == 8) return launch_attn<T, 4, 4, true, false>(a);
    } else {
        if (a.wse == 24) return launch_attn<T, 36, 12, false, false>(a);
        if (a.wse == 12) return launch_attn<T, 9, 9, false, false>(a);
        if (a.wse == 25) return launch_attn<T, 40, 10, false, true>(a);
        if (a.wse == 13) return launch_attn<T, 11, 11, false, true>(a);
    }
    return HAT_EUNSUPPORTED;  // other window sizes are not instantiated
}

template <bool SELF>
int attn_dispatch(const AttnArgs& a, int dtype) {
    if (dtype == HAT_BF16) return attn_by_window<bf16_t, SELF>(a);
    if (dtype == HAT_F32) return attn_by_window<float, SELF>(a);
    return HAT_EINVAL;
}
}  // namespace


static int ocab_attention_impl(const void* q, const void* kv, const float* bias_rot, void* out, int32_t B, int32_t H,
                               int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t ldq,
                               int32_t ldkv, int32_t ldo, int32_t dtype, void* stream, bool qlog2) {
    if (const int rc = attn_check(q && kv && bias_rot && out, B, C, heads, ldq, ldkv, ldo,
                                  [&] { return !(ws < 4 || H % ws || W % ws || wse < ws || (ws * ws) % 16); }))
        return rc;
    const int d = C / heads;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (the pointer term as in hat_window_attention: the D = 24 kernel stages q / k / v in 16-byte pieces and stores 8-byte ones, so
    // the strides alone do not make its accesses aligned; a call that misses it takes the generic kernel — the log2 entry refuses)
    const bool fast24 = d == 24 && ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0 && C % 8 == 0 &&
                        (reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv)) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0;
    const bool fast30 = d == 30 && ldq % 2 == 0 && ldkv % 2 == 0 && ldo % 2 == 0 && C % 2 == 0 &&   // (4-byte accesses throughout)
                        (reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out)) % 4 == 0;
    if (dtype == HAT_BF16 && ws == 16 && wse == 24 && (fast24 || fast30)) {
        // (always above 64 KiB: the limit is raised on every call)
        const size_t lds = (size_t)576 * ((fast24 && !qlog2) ? 24 : 32) * 2 + (size_t)576 * 32 * 2 + (size_t)39 * 39 * 4;
        if (qlog2 && !fast24) return HAT_EUNSUPPORTED;
        auto kern = fast24 ? (qlog2 ? ocab_attn_fast_kernel<24, 24, false, 512, true> : ocab_attn_fast_kernel<24, 24, false, 512>)
                           : ocab_attn_fast_kernel<30, 24, false, 512>;
        const int nwin = B * (W / ws) * (H / ws);
        return attn_launch(kern, dim3((nwin + 7) / 8 * 8 * heads), 512, lds, s, reinterpret_cast<const bf16_t*>(q),
                           reinterpret_cast<const bf16_t*>(kv), bias_rot, reinterpret_cast<bf16_t*>(out), B, H, W, C, heads, ldq, ldkv, ldo, 0);
    }
    if (qlog2) return HAT_EUNSUPPORTED;   // only the tuned kernel takes log2-domain queries
    return attn_dispatch<false>(AttnArgs{q, kv, bias_rot, out, B, H, W, C, heads, ws, wse, ldq, ldkv, ldo, s, 0, nullptr, -1}, dtype);
}

extern "C" int hat_ocab_attention(const void* q, const void* kv, const float* bias_rot, void* out, int32_t B, int32_t H,
                                  int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t ldq,
                                  int32_t ldkv, int32_t ldo, int32_t dtype, void* stream) {
    return ocab_attention_impl(q, kv, bias_rot, out, B, H, W, C, heads, ws, wse, ldq, ldkv, ldo, dtype, stream, false);
}

extern "C" int hat_ocab_attention_log2(const void* q, const void* kv, const float* bias_rot, void* out, int32_t B, int32_t H,
                                       int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t ldq,
                                       int32_t ldkv, int32_t ldo, int32_t dtype, void* stream) {
    return ocab_attention_impl(q, kv, bias_rot, out, B, H, W, C, heads, ws, wse, ldq, ldkv, ldo, dtype, stream, true);
}

extern "C" int hat_ocab_keybias(const void* sal, int32_t ldsal, const void* kv, int32_t ldkv, float* kb, int32_t B, int32_t H, int32_t W,
                                int32_t C, int32_t ws, int32_t wse, int32_t pad, int32_t k_keep, int32_t dtype, void* stream) {
    if (!kb || (!sal && !kv) || B < 1 || ws < 1 || H % ws || W % ws || wse < ws || wse * wse > 1024 || pad < 0 || k_keep < 1) return HAT_EINVAL;
    if ((sal && ldsal == 0) || (sal && ldsal < 0 && dtype != HAT_BF16) || (!sal && ldkv < C)) return HAT_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid(W / ws, H / ws, B);
    if (dtype == HAT_BF16 && sal && ldsal < 0)   // ldsal < 0: the saliency map is FP32 with row stride -ldsal (the keys are ranked on it)
        HAT_LAUNCH((keybias_kernel<bf16_t, float>), grid, dim3(1024), 0, s, reinterpret_cast<const float*>(sal), -ldsal, reinterpret_cast<const bf16_t*>(kv),
                   ldkv, kb, H, W, C, ws, wse, pad, k_keep);
    else if (dtype == HAT_BF16)
        HAT_LAUNCH(keybias_kernel<bf16_t>, grid, dim3(1024), 0, s, reinterpret_cast<const bf16_t*>(sal), ldsal, reinterpret_cast<const bf16_t*>(kv), ldkv, kb,
                   H, W, C, ws, wse, pad, k_keep);
    else if (dtype == HAT_F32)
        HAT_LAUNCH(keybias_kernel<float>, grid, dim3(1024), 0, s, reinterpret_cast<const float*>(sal), ldsal, reinterpret_cast<const float*>(kv), ldkv, kb, H, W,
                   C, ws, wse, pad, k_keep);
    else
        return HAT_EINVAL;
    return hat_check_launch();
}

extern "C" int hat_ocab_attention_kb(const void* q, const void* kv, const float* bias_rot, const float* kb, void* out, int32_t B, int32_t H,
                                     int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t wse, int32_t pad, int32_t ldq, int32_t ldkv,
                                     int32_t ldo, int32_t dtype, void* stream) {
    if (const int rc = attn_check(q && kv && bias_rot && kb && out, B, C, heads, ldq, ldkv, ldo, [&] {
            return !(ws < 4 || H % ws || W % ws || wse < ws || (ws * ws) % 16 || pad != (wse - ws + 1) / 2);
        }))
        return rc;
    return attn_dispatch<false>(
        AttnArgs{q, kv, bias_rot, out, B, H, W, C, heads, ws, wse, ldq, ldkv, ldo, reinterpret_cast<hipStream_t>(stream), 0, kb, pad}, dtype);
}

extern "C" int hat_window_attention(const void* q, const void* kv, const float* bias_flip, void* out, int32_t B, int32_t H,
                                    int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t shift, int32_t ldq,
                                    int32_t ldkv, int32_t ldo, int32_t dtype, void* stream) {
    if (const int rc = attn_check(q && kv && bias_flip && out, B, C, heads, ldq, ldkv, ldo,
                                  [&] { return !(ws < 4 || ws % 4 || H % ws || W % ws || shift < 0 || shift >= ws || shift % 4); }))
        return rc;
    const int d = C / heads;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool fast24 = d == 24 && ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0 && C % 8 == 0 &&
                        (reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv)) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0;
    const bool fast30 = d == 30 && ldq % 2 == 0 && ldkv % 2 == 0 && ldo % 2 == 0 && C % 2 == 0 &&   // (4-byte accesses throughout)
                        (reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out)) % 4 == 0;
    if (dtype == HAT_BF16 && ws == 16 && (fast24 || fast30)) {
        // (36 612 B at most: the limit is never raised)
        const size_t lds = (size_t)256 * (fast24 ? 24 : 32) * 2 + (size_t)256 * 32 * 2 + (size_t)31 * 31 * 4;
        auto kern = fast24 ? ocab_attn_fast_kernel<24, 16, true> : ocab_attn_fast_kernel<30, 16, true>;
        const int nwin = B * (W / ws) * (H / ws);
        return attn_launch(kern, dim3((nwin + 7) / 8 * 8 * heads), 256, lds, s, reinterpret_cast<const bf16_t*>(q),
                           reinterpret_cast<const bf16_t*>(kv), bias_flip, reinterpret_cast<bf16_t*>(out), B, H, W, C, heads, ldq, ldkv,
                           ldo, shift);
    }
    return attn_dispatch<true>(AttnArgs{q, kv, bias_flip, out, B, H, W, C, heads, ws, ws, ldq, ldkv, ldo, s, shift, nullptr, -1}, dtype);
}
