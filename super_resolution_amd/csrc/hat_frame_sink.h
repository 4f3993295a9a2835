// hat_frame_sink.h — the frame sink: what every kernel that ends in interleaved bytes or in a YCbCr surface shares after its RGB
// values are in registers.  The arithmetic is hat_common.h's and the sample types are hat_yuv_sample.h's; here are the typed
// destination (HatYuvDst), the stores of a thread that owns an R x 4 tile (yuv_store_tile) or four pixels of a row
// (rgb4_store_u8), the stores of a lane that owns one pixel (yuv_store_luma, yuv_store_chroma420 / 422 / 444) and the host's
// choice of instance (yuv_dispatch).
// Included by hat_yuv.hip and hat_u8.hip (planes in), hat_esc_sink.hip (shuffled rows in), hat_lte.hip (hat_lte_query's sink) and
// hat_cabsq.hip (conv_last's row sweep).  A new sink brings its values to one of the two thread shapes and calls these; how a
// partner's chroma term reaches the lane that stores stays the kernel's own.  HIP sources only.
#pragma once
#include "hat_common.h"
#include "hat_yuv_check.h"
#include "hat_yuv_sample.h"

namespace {

// A HatYuvSurface with its pointers typed: T = uint8_t or uint16_t (const T for a source).  Pitches, batch strides and the
// chroma step are in bytes for every T.  cb = cr = null: grey.
template <typename T> struct HatYuvDst {
    T* y;
    T* cb;
    T* cr;
    long long y_pitch, y_bstride, c_pitch, c_bstride;
    int c_step;
    __device__ __forceinline__ T& luma(int b, int row, int col) const {
        return sample_at(y, (size_t)b * y_bstride + (size_t)row * y_pitch + (size_t)col * sizeof(T));
    }
    // byte offset of chroma sample (row, col) of the chroma planes: the same for cb and cr
    __device__ __forceinline__ size_t chroma(int b, int row, int col) const { return (size_t)b * c_bstride + (size_t)row * c_pitch + (size_t)col * c_step; }
};

template <typename T> HatYuvDst<T> yuv_dst(const HatYuvSurface& s) {
    return HatYuvDst<T>{reinterpret_cast<T*>(s.y), reinterpret_cast<T*>(s.cb), reinterpret_cast<T*>(s.cr), (long long)s.y_pitch,
                        (long long)s.y_bstride, (long long)s.c_pitch, (long long)s.c_bstride, (int)s.c_step};
}

// ---- a lane owns one pixel ----------------------------------------------------------------------------------------------------
// Y of pixel (row, col); the chroma sample (row, col) of the chroma planes from the per-pixel terms cb, cr of hat_rgb_to_ycc:
// 4:2:0 from the pair sums (left + right) of the block's top and bottom row, 4:2:2 from the pair's sum, 4:4:4 from the pixel's term.
template <typename T> __device__ __forceinline__ void yuv_store_luma(const HatYuvDst<T>& d, const HatSample<T>& q, int b, int row, int col, float Y) {
    d.luma(b, row, col) = (T)q.luma(Y);
}

template <typename T>
__device__ __forceinline__ void yuv_store_chroma420(const HatYuvDst<T>& d, const HatSample<T>& q, const HatCsc& k, int b, int row, int col,
                                                    float top_b, float bottom_b, float top_r, float bottom_r) {
    const size_t co = d.chroma(b, row, col);
    sample_at(d.cb, co) = (T)q.chroma(top_b, bottom_b, k.m[7]);
    sample_at(d.cr, co) = (T)q.chroma(top_r, bottom_r, k.m[11]);
}

template <typename T>
__device__ __forceinline__ void yuv_store_chroma422(const HatYuvDst<T>& d, const HatSample<T>& q, const HatCsc& k, int b, int row, int col,
                                                    float sum_b, float sum_r) {
    const size_t co = d.chroma(b, row, col);
    sample_at(d.cb, co) = (T)q.luma(hat_chroma_value_h(sum_b, k.m[7]));
    sample_at(d.cr, co) = (T)q.luma(hat_chroma_value_h(sum_r, k.m[11]));
}

template <typename T>
__device__ __forceinline__ void yuv_store_chroma444(const HatYuvDst<T>& d, const HatSample<T>& q, const HatCsc& k, int b, int row, int col, float cb,
                                                    float cr) {
    const size_t co = d.chroma(b, row, col);
    sample_at(d.cb, co) = (T)q.luma(hat_add_rn(cb, k.m[7]));
    sample_at(d.cr, co) = (T)q.luma(hat_add_rn(cr, k.m[11]));
}

// ---- a thread owns (1 + SUB_Y) rows x four columns at (y, x) -------------------------------------------------------------------
// (4:2:0: two 2 x 2 blocks, rows are not independent there.)  load(rgb) fills the tile: rgb[j][i] is pixel (y + j, x + i); the
// columns i >= n are not read (a row's tail: n = 1, 2 or 3, odd only without horizontal subsampling).  The tile is this function's
// own array and not the caller's: with the caller's array the compiler issues every load of a 4:2:0 tile before the first
// conversion and the kernels need four times the registers.  The four Y samples of a row go out through store_row4.
// 4:2:0 and 4:2:2: the two Cb and two Cr samples are single stores (planar or interleaved: the step decides), from the pair sums
// left + right, then top + bottom; 4:4:4: four samples a row, through store_row4 when planar.
template <typename T, int SUB_X, int SUB_Y, bool GREY, typename Load>
__device__ __forceinline__ void yuv_store_tile(const HatYuvDst<T>& d, const HatCsc& k, const HatSample<T>& q, int b, int y, int x, int n, Load&& load) {
    constexpr int R = 1 + SUB_Y;
    float rgb[R][4][3];
    load(rgb);
    float cb[R][4], cr[R][4];
    unsigned v[R][4];
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float Y = 0.f;
            cb[j][i] = cr[j][i] = 0.f;
            if (i < n) hat_rgb_to_ycc(k, rgb[j][i][0], rgb[j][i][1], rgb[j][i][2], Y, cb[j][i], cr[j][i]);
            v[j][i] = q.luma(Y);
        }
#pragma unroll
    for (int j = 0; j < R; ++j) store_row4(&d.luma(b, y + j, x), v[j], n);
    if constexpr (!GREY && SUB_X == 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (2 * i < n) {
                const float sb = hat_add_rn(cb[0][2 * i], cb[0][2 * i + 1]), sr = hat_add_rn(cr[0][2 * i], cr[0][2 * i + 1]);
                if constexpr (SUB_Y == 1)
                    yuv_store_chroma420(d, q, k, b, y >> 1, (x >> 1) + i, sb, hat_add_rn(cb[1][2 * i], cb[1][2 * i + 1]), sr,
                                        hat_add_rn(cr[1][2 * i], cr[1][2 * i + 1]));
                else
                    yuv_store_chroma422(d, q, k, b, y, (x >> 1) + i, sb, sr);
            }
        }
    } else if constexpr (!GREY) {
        unsigned vb[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            vb[i] = q.luma(hat_add_rn(cb[0][i], k.m[7]));
            vr[i] = q.luma(hat_add_rn(cr[0][i], k.m[11]));
        }
        const size_t co = d.chroma(b, y, x);
        if (d.c_step == (int)sizeof(T)) {
            store_row4(&sample_at(d.cb, co), vb, n);
            store_row4(&sample_at(d.cr, co), vr, n);
        } else {
            for (int i = 0; i < n; ++i) {
                sample_at(d.cb, co + (size_t)i * d.c_step) = (T)vb[i];
                sample_at(d.cr, co + (size_t)i * d.c_step) = (T)vr[i];
            }
        }
    }
}

// four consecutive pixels of a row as interleaved bytes at o: tensor2img's quantisation (hat_unit_to_u8), bytes 0 and 2 of a
// pixel swapped with bgr; three dword stores when all four are there and o is 4-byte aligned, single bytes otherwise (the last
// segment of a row, odd pitches).  The columns i >= n are not read.
__device__ __forceinline__ void rgb4_store_u8(uint8_t* o, const float (&rgb)[4][3], int n, int bgr) {
    unsigned q[12];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) q[3 * i + c] = i < n ? hat_unit_to_u8(bgr ? rgb[i][2 - c] : rgb[i][c]) : 0u;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<unsigned*>(o)[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | (q[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) o[k] = (uint8_t)q[k];
    }
}

// ---- the host's choice of instance ---------------------------------------------------------------------------------------------
// What a surface fixes at compile time: the sample type, log2 of the chroma subsampling ((1,1) 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4)
// and grey (no chroma planes).
template <typename T, int SX, int SY, bool GREY> struct HatYuvLayout {
    using sample_t = T;
    static constexpr int sx = SX, sy = SY;
    static constexpr bool grey = GREY;
};

// f(HatSample<T>) by the surface's depth
template <typename F> auto yuv_dispatch_depth(const HatYuvSurface& s, F&& f) {
    if (s.depth == 8) return f(HatSample<uint8_t>{});
    return f(deep_sample(s.depth, s.msb));
}

// f(HatYuvLayout<T, SX, SY, GREY>, HatSample<T>) by the surface's depth and subsampling; returns what f returns
template <typename F> auto yuv_dispatch(const HatYuvSurface& s, F&& f) {
    return yuv_dispatch_depth(s, [&](auto q) {
        using T = typename decltype(q)::sample_t;
        if (!s.cb) return f(HatYuvLayout<T, 0, 0, true>{}, q);
        if (s.sub_y) return f(HatYuvLayout<T, 1, 1, false>{}, q);
        if (s.sub_x) return f(HatYuvLayout<T, 1, 0, false>{}, q);
        return f(HatYuvLayout<T, 0, 0, false>{}, q);
    });
}

}  // namespace
