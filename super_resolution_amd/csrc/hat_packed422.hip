// hat_packed422.hip — packed 4:2:2 frames (UYVY, YUY2: bytes; Y210 / Y216: 16-bit words; v210: three 10-bit codes a dword) <->
// the network's fp32 RGB planes.  Contract: include/hat_mi355x.h, "Packed 4:2:2"; definition: super_resolution_amd/yuv.py
// (packed_to_planes, planes_to_packed).  A packed sample means what the sample of a (sub_x, sub_y) = (1, 0) surface means, so
// only the addressing is here: every value goes through hat_yuv.hip's own steps — HatSample<T>'s to_rgb / value / luma,
// hat_chroma_up4, hat_rgb_to_ycc, hat_chroma_value_h, hat_chroma_tap121 / hat_chroma_value_s — in the order the 4:2:2
// instances of that file take them, and the results equal theirs bit for bit.
#include "hat_packed_check.h"
#include "hat_yuv_check.h"
#include "hat_yuv_sample.h"

namespace {

typedef unsigned u32x2a __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned u32x4a __attribute__((ext_vector_type(4), aligned(4)));

// Where the samples of a row lie, per layout.  sample_t: the HatSample the values go through (v210's codes are LSB-aligned
// 10-bit words to it).  PAIRS, UNIT: pixel pairs and bytes of the unit a lane of the out kernel owns.
// luma(row, x): the stored Y of pixel x; cb / cr(row, j): the stored chroma of pair j.  unit(o, Y, Cb, Cr): the unit's words.
template <int YOFF, int COFF> struct PackedBytes {   // Y at byte 4 j + YOFF (+ 2), Cb at 4 j + COFF, Cr at 4 j + COFF + 2
    using sample_t = uint8_t;
    static constexpr int PAIRS = 1, UNIT = 4;
    static __device__ __forceinline__ unsigned luma(const char* row, int x) { return (uint8_t)row[4 * (x >> 1) + YOFF + 2 * (x & 1)]; }
    static __device__ __forceinline__ unsigned cb(const char* row, int j) { return (uint8_t)row[4 * j + COFF]; }
    static __device__ __forceinline__ unsigned cr(const char* row, int j) { return (uint8_t)row[4 * j + COFF + 2]; }
    static __device__ __forceinline__ void unit(char* o, const unsigned (&Y)[2], const unsigned (&Cb)[1], const unsigned (&Cr)[1]) {
        *reinterpret_cast<unsigned*>(o) = (Y[0] << (8 * YOFF)) | (Y[1] << (8 * YOFF + 16)) | (Cb[0] << (8 * COFF)) | (Cr[0] << (8 * COFF + 16));
    }
};
struct PackedWords {   // Y210: words Y0 Cb Y1 Cr
    using sample_t = uint16_t;
    static constexpr int PAIRS = 1, UNIT = 8;
    static __device__ __forceinline__ unsigned word(const char* row, int i) { return reinterpret_cast<const uint16_t*>(row)[i]; }
    static __device__ __forceinline__ unsigned luma(const char* row, int x) { return word(row, 2 * x); }
    static __device__ __forceinline__ unsigned cb(const char* row, int j) { return word(row, 4 * j + 1); }
    static __device__ __forceinline__ unsigned cr(const char* row, int j) { return word(row, 4 * j + 3); }
    static __device__ __forceinline__ void unit(char* o, const unsigned (&Y)[2], const unsigned (&Cb)[1], const unsigned (&Cr)[1]) {
        if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<u32x2a*>(o) = u32x2a{Y[0] | (Cb[0] << 16), Y[1] | (Cr[0] << 16)};
        } else {   // a surface aligned to its words only: the same lane stores the four of them
            uint16_t* p = reinterpret_cast<uint16_t*>(o);
            p[0] = (uint16_t)Y[0], p[1] = (uint16_t)Cb[0], p[2] = (uint16_t)Y[1], p[3] = (uint16_t)Cr[0];
        }
    }
};
struct PackedV210 {   // component n of a group of six pixels (Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 Cb2 Y4 Cr2 Y5): dword n / 3, bit 10 (n % 3)
    using sample_t = uint16_t;
    static constexpr int PAIRS = 3, UNIT = 16;
    static __device__ __forceinline__ unsigned comp(const char* row, int g, int n) {
        return (reinterpret_cast<const unsigned*>(row)[4 * g + n / 3] >> (10 * (n % 3))) & 1023u;
    }
    static __device__ __forceinline__ unsigned luma(const char* row, int x) { return comp(row, x / 6, 2 * (x % 6) + 1); }
    static __device__ __forceinline__ unsigned cb(const char* row, int j) { return comp(row, j / 3, 4 * (j % 3)); }
    static __device__ __forceinline__ unsigned cr(const char* row, int j) { return comp(row, j / 3, 4 * (j % 3) + 2); }
    static __device__ __forceinline__ void unit(char* o, const unsigned (&Y)[6], const unsigned (&Cb)[3], const unsigned (&Cr)[3]) {
        *reinterpret_cast<u32x4a*>(o) = u32x4a{Cb[0] | (Y[0] << 10) | (Cr[0] << 20), Y[1] | (Cb[1] << 10) | (Y[2] << 20),
                                               Cr[1] | (Y[3] << 10) | (Cb[2] << 20), Y[4] | (Cr[2] << 10) | (Y[5] << 20)};
    }
};

struct PackedRows {   // a HatPackedSurface's addressing: bytes
    char* base;
    long long pitch, bstride;
    __device__ __forceinline__ char* row(int b, int y) const { return base + (size_t)b * bstride + (size_t)y * pitch; }
};

// one thread = one pixel of the padded plane row, as in yuv420_to_planes_kernel / yuv_to_planes_sited_kernel<T, 0, 1>: the
// reflection, then the pixel's Y and the chroma of its pair (SITED: of pairs j and min(j + (x & 1), cw - 1)).
template <typename L, bool SITED>
__global__ __launch_bounds__(256) void packed422_to_planes_kernel(const PackedRows s, float* __restrict__ dst, int h, int w, int Hp, int Wp, HatCsc k,
                                                                  HatSample<typename L::sample_t> q) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    const char* row = s.row(b, sy);
    const int j = sx >> 1;
    float rgb[3];
    if constexpr (SITED) {
        const int j1 = min(j + (sx & 1), (w >> 1) - 1);
        const float Y = q.value(L::luma(row, sx));
        const float b0 = q.value(L::cb(row, j)), b1 = q.value(L::cb(row, j1)), r0 = q.value(L::cr(row, j)), r1 = q.value(L::cr(row, j1));
        hat_ycc_to_rgb_f(k, Y, hat_chroma_up4(b0, b1, b0, b1), hat_chroma_up4(r0, r1, r0, r1), rgb);
    } else {
        q.to_rgb(k, L::luma(row, sx), L::cb(row, j), L::cr(row, j), rgb);
    }
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = rgb[c];
}

// one lane = one unit of a destination row: L::PAIRS pixel pairs from column x, no two lanes write the same word.  SITED: the
// lane also converts column max(x - 1, 0), the left tap of its first pair (planes_to_yuv_sited_kernel's column 0).  v210: the
// pairs of the last group that lie past w_out are zero codes, and the lane of the last group zeroes the row from there to
// row_bytes, the end of the layout's row; nothing past row_bytes is written.
template <typename L, bool SITED>
__global__ __launch_bounds__(256) void planes_to_packed422_kernel(const float* __restrict__ src, int Hs, int Ws, const PackedRows d, int w_out,
                                                                  int row_bytes, HatCsc k, HatSample<typename L::sample_t> q) {
    constexpr int P = L::PAIRS, N = 2 * P;
    const int u = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int x = u * N;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* sr = src + (size_t)b * 3 * plane + (size_t)y * Ws;
    const int n = min(N, w_out - x);   // even
    float cb[N + 1], cr[N + 1];        // column 0: image column max(x - 1, 0) (SITED only); column 1 + i: x + i
    unsigned Y[N], Cb[P], Cr[P];
#pragma unroll
    for (int i = SITED ? 0 : 1; i < N + 1; ++i) {
        const int col = max(x + i - 1, 0);
        float Yf = 0.f;
        cb[i] = cr[i] = 0.f;
        if (i - 1 < n) hat_rgb_to_ycc(k, sr[col], sr[plane + col], sr[2 * plane + col], Yf, cb[i], cr[i]);
        if (i >= 1) Y[i - 1] = i - 1 < n ? q.luma(Yf) : 0u;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        Cb[p] = Cr[p] = 0u;
        if (2 * p < n) {
            if constexpr (SITED) {
                Cb[p] = q.luma(hat_chroma_value_s(hat_chroma_tap121(cb[2 * p], cb[2 * p + 1], cb[2 * p + 2]), 0.25f, k.m[7]));
                Cr[p] = q.luma(hat_chroma_value_s(hat_chroma_tap121(cr[2 * p], cr[2 * p + 1], cr[2 * p + 2]), 0.25f, k.m[11]));
            } else {
                Cb[p] = q.luma(hat_chroma_value_h(hat_add_rn(cb[2 * p + 1], cb[2 * p + 2]), k.m[7]));
                Cr[p] = q.luma(hat_chroma_value_h(hat_add_rn(cr[2 * p + 1], cr[2 * p + 2]), k.m[11]));
            }
        }
    }
    char* row = d.row(b, y);
    constexpr int UNIT = L::UNIT;
    L::unit(row + (size_t)u * UNIT, Y, Cb, Cr);
    if constexpr (P == 3) {
        if (x + N >= w_out)
            for (int o = (u + 1) * UNIT; o < row_bytes; o += UNIT) *reinterpret_cast<u32x4a*>(row + o) = u32x4a{0u, 0u, 0u, 0u};
    }
}

// f(layout traits, HatSample) by the surface's layout
template <typename F> void packed_dispatch(const HatPackedSurface& s, F&& f) {
    if (s.layout == HAT_PACKED_UYVY) f(PackedBytes<1, 0>{}, HatSample<uint8_t>{});
    else if (s.layout == HAT_PACKED_YUY2) f(PackedBytes<0, 1>{}, HatSample<uint8_t>{});
    else if (s.layout == HAT_PACKED_Y210) f(PackedWords{}, deep_sample(s.depth, s.msb));
    else f(PackedV210{}, deep_sample(10, 0));
}

PackedRows packed_rows(const HatPackedSurface& s) { return PackedRows{reinterpret_cast<char*>(s.base), (long long)s.pitch, (long long)s.bstride}; }

}  // namespace

extern "C" int hat_packed422_to_planes(const HatPackedSurface* src, int32_t siting, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp,
                                       int32_t Wp, const float* to_rgb12, void* stream) {
    if (!hat_siting_ok(siting) || !dst || !to_rgb12 || !hat_packed_surface_ok(src, B, h, w) || !hat_packed_padded_ok(B, h, w, Hp, Wp))
        return HAT_EINVAL;
    packed_dispatch(*src, [&](auto L, auto q) {
        using T = decltype(L);
        const dim3 grid((Wp + 255) / 256, Hp, B);
        if (siting == HAT_SITING_CENTER)
            HAT_LAUNCH((packed422_to_planes_kernel<T, false>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), packed_rows(*src), dst, h, w,
                       Hp, Wp, load_csc(to_rgb12), q);
        else
            HAT_LAUNCH((packed422_to_planes_kernel<T, true>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), packed_rows(*src), dst, h, w,
                       Hp, Wp, load_csc(to_rgb12), q);
    });
    return hat_check_launch();
}

extern "C" int hat_planes_to_packed422(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatPackedSurface* dst, int32_t siting,
                                       int32_t h_out, int32_t w_out, const float* from_rgb12, void* stream) {
    if (!hat_siting_ok(siting) || !src || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_packed_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out > 65535) return HAT_EINVAL;
    const int row_bytes = (int)hat_packed_row_bytes(dst->layout, w_out);
    packed_dispatch(*dst, [&](auto L, auto q) {
        using T = decltype(L);
        const int units = (w_out + 2 * T::PAIRS - 1) / (2 * T::PAIRS);
        const dim3 grid((units + 255) / 256, h_out, B);
        if (siting == HAT_SITING_CENTER)
            HAT_LAUNCH((planes_to_packed422_kernel<T, false>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, Hs, Ws,
                       packed_rows(*dst), w_out, row_bytes, load_csc(from_rgb12), q);
        else
            HAT_LAUNCH((planes_to_packed422_kernel<T, true>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, Hs, Ws,
                       packed_rows(*dst), w_out, row_bytes, load_csc(from_rgb12), q);
    });
    return hat_check_launch();
}
