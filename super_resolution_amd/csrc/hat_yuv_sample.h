// hat_yuv_sample.h — what the kernels that read or write YCbCr samples share beyond hat_common.h's arithmetic: the sample types
// (bytes, n-bit codes in 16-bit words), byte addressing of a sample, and the host side's matrix and deep-sample arguments.
// Included through hat_frame_sink.h, which holds the stores built on these.  HIP sources only.
#pragma once
#include <type_traits>

#include "hat_common.h"

namespace {

// What differs between the sample types T.  uint8_t: nothing travels.  uint16_t: an n-bit code in a 16-bit word —
// shift = 16 - n for MSB-aligned words (else 0), maxcode = 2^n - 1, inv = 2^(8 - n), scale = 2^(n - 8).
template <typename T> struct HatSample;
template <> struct HatSample<uint8_t> {
    using sample_t = uint8_t;
    __device__ __forceinline__ void to_rgb(const HatCsc& k, unsigned Y, unsigned Cb, unsigned Cr, float (&rgb)[3]) const { hat_ycc_to_rgb(k, Y, Cb, Cr, rgb); }
    __device__ __forceinline__ unsigned luma(float v) const { return hat_ycc_byte(v); }
    __device__ __forceinline__ unsigned chroma(float top, float bottom, float offset) const { return hat_chroma_byte(top, bottom, offset); }
    __device__ __forceinline__ unsigned neutral() const { return 128u; }   // the chroma sample of a grey frame: Cb' = Cr' = 0
    __device__ __forceinline__ float value(unsigned word) const { return (float)word; }   // the sample in byte units (sited kernels)
};
template <> struct HatSample<uint16_t> {
    using sample_t = uint16_t;
    int shift;
    unsigned maxcode;
    float inv, scale;
    __device__ __forceinline__ unsigned code(unsigned word) const { return min(word >> shift, maxcode); }   // LSB words above the range saturate
    __device__ __forceinline__ void to_rgb(const HatCsc& k, unsigned Y, unsigned Cb, unsigned Cr, float (&rgb)[3]) const {
        hat_ycc_to_rgb(k, code(Y), code(Cb), code(Cr), inv, rgb);
    }
    __device__ __forceinline__ unsigned luma(float v) const { return hat_ycc_code(v, scale, (float)maxcode) << shift; }
    __device__ __forceinline__ unsigned chroma(float top, float bottom, float offset) const {
        return hat_ycc_code(hat_chroma_value(top, bottom, offset), scale, (float)maxcode) << shift;
    }
    __device__ __forceinline__ unsigned neutral() const { return (128u * (unsigned)scale) << shift; }
    __device__ __forceinline__ float value(unsigned word) const { return (float)code(word) * inv; }   // exact: code * 2^-k
};

// sample i of a row that starts at byte address p (pitches, strides and the chroma step are in bytes for every T)
template <typename T> __device__ __forceinline__ T& sample_at(T* base, size_t bytes) {
    using byte_t = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return *reinterpret_cast<T*>(reinterpret_cast<byte_t*>(base) + bytes);
}

// four samples of one row from o: one store (a dword of bytes, 8 bytes of words) where all four are there and o is aligned to
// that store, single samples otherwise
template <typename T> __device__ __forceinline__ void store_row4(T* o, const unsigned (&v)[4], int n) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<unsigned*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u32x2*>(o) = u32x2{v[0] | (v[1] << 16), v[2] | (v[3] << 16)};
        }
    } else {
        for (int i = 0; i < n; ++i) o[i] = (T)v[i];
    }
}

HatCsc load_csc(const float* m12) {
    HatCsc k;
    for (int i = 0; i < 12; ++i) k.m[i] = m12[i];
    return k;
}

HatSample<uint16_t> deep_sample(int depth, int msb) {
    return HatSample<uint16_t>{msb ? 16 - depth : 0, (1u << depth) - 1u, 1.0f / (float)(1 << (depth - 8)), (float)(1 << (depth - 8))};
}

}  // namespace
