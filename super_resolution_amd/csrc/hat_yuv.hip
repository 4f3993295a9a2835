// hat_yuv.hip — the 4:2:0 frame boundary: YCbCr frames (NV12 / NV21 / I420, bytes; P010 / P012 / P016 / yuv420p1xle, 16-bit
// words) <-> the network's fp32 RGB planes.  Contract: include/hat_mi355x.h (hat_yuv420_to_planes, hat_planes_to_yuv420 and
// their p16 forms); definition: super_resolution_amd/yuv.py;
// colour conversion: basicsr utils/color_util.py (rgb2ycbcr, ycbcr2rgb: BT.601, 16-235), shared with conv_last's yuv epilogue
// through hat_common.h (hat_ycc_to_rgb, hat_rgb_to_ycc).  cb and cr are separate pointers with a byte step between the
// samples of a row (1: planar, 2: interleaved), so one kernel serves all three layouts.  The chroma subsampling (SUB_X, SUB_Y) and
// grey (no chroma) are template parameters of the same two kernels: (1,1) is 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4; the surface
// entries (hat_yuv_to_planes, hat_planes_to_yuv) pick the instance.  Those are centre-sited chroma (nearest up, box down); the
// co-sited instances ('left', 'topleft': hat_yuv_to_planes_sited, hat_planes_to_yuv_sited) are kernels of their own beside them.
#include "hat_common.h"
#include "hat_yuv_check.h"
#include "hat_yuv_sample.h"

namespace {

// one thread = one pixel of the padded plane row (hat_u8_to_planes' shape): a Y sample, the Cb and Cr samples of its 2 x 2 block
// (the four pixels of a block read the same two samples: L1), three plane stores coalesced over the lanes.  Reflection as in
// u8_to_planes_kernel; the chroma sample of source pixel (sy, sx) is (sy >> SUB_Y, sx >> SUB_X).  GREY: no chroma is read, both
// samples are the neutral one.
template <typename T, int SUB_X, int SUB_Y, bool GREY>
__global__ __launch_bounds__(256) void yuv420_to_planes_kernel(const T* __restrict__ yp, long long y_pitch, long long y_bstride,
                                                               const T* __restrict__ cbp, const T* __restrict__ crp,
                                                               long long c_pitch, int c_step, long long c_bstride, float* __restrict__ dst,
                                                               int h, int w, int Hp, int Wp, HatCsc k, HatSample<T> q) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    float rgb[3];
    const unsigned Yw = sample_at(yp, (size_t)b * y_bstride + (size_t)sy * y_pitch + (size_t)sx * sizeof(T));
    if constexpr (GREY) {
        q.to_rgb(k, Yw, q.neutral(), q.neutral(), rgb);
    } else {
        const size_t co = (size_t)b * c_bstride + (size_t)(sy >> SUB_Y) * c_pitch + (size_t)(sx >> SUB_X) * c_step;
        q.to_rgb(k, Yw, sample_at(cbp, co), sample_at(crp, co), rgb);
    }
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = rgb[c];
}

// The same thread shape for co-sited chroma (yuv.py, "Chroma siting"; SUB_X = 1 always): SITING 1 ('left') interpolates along x,
// SITING 2 ('topleft', SUB_Y = 1 only) along y too.  An odd source column reads its two neighbours j, min(j + 1, cw - 1), an odd
// source row i, min(i + 1, ch - 1): up to four samples a plane, all inside the (ch, cw) chroma plane.
template <typename T, int SUB_Y, int SITING>
__global__ __launch_bounds__(256) void yuv_to_planes_sited_kernel(const T* __restrict__ yp, long long y_pitch, long long y_bstride,
                                                                  const T* __restrict__ cbp, const T* __restrict__ crp,
                                                                  long long c_pitch, int c_step, long long c_bstride, float* __restrict__ dst,
                                                                  int h, int w, int Hp, int Wp, HatCsc k, HatSample<T> q) {
    static_assert(SITING == 1 || (SITING == 2 && SUB_Y == 1), "a co-sited row axis needs vertical subsampling");
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    const int cw = w >> 1, ch = h >> SUB_Y;
    const int j = sx >> 1, j1 = min(j + (sx & 1), cw - 1);
    const int i = sy >> SUB_Y, i1 = SITING == 2 ? min(i + (sy & 1), ch - 1) : i;
    const float Y = q.value(sample_at(yp, (size_t)b * y_bstride + (size_t)sy * y_pitch + (size_t)sx * sizeof(T)));
    const size_t r0 = (size_t)b * c_bstride + (size_t)i * c_pitch, r1 = (size_t)b * c_bstride + (size_t)i1 * c_pitch;
    const size_t o0 = (size_t)j * c_step, o1 = (size_t)j1 * c_step;
    const float cb = hat_chroma_up4(q.value(sample_at(cbp, r0 + o0)), q.value(sample_at(cbp, r0 + o1)), q.value(sample_at(cbp, r1 + o0)),
                                    q.value(sample_at(cbp, r1 + o1)));
    const float cr = hat_chroma_up4(q.value(sample_at(crp, r0 + o0)), q.value(sample_at(crp, r0 + o1)), q.value(sample_at(crp, r1 + o0)),
                                    q.value(sample_at(crp, r1 + o1)));
    float rgb[3];
    hat_ycc_to_rgb_f(k, Y, cb, cr, rgb);
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = rgb[c];
}

// one thread = (1 + SUB_Y) rows x four columns (4:2:0: two 2 x 2 blocks, rows are not independent there).  Per row and plane 16
// contiguous bytes are loaded; the four Y samples of a row go out through store_row4.  4:2:0 and 4:2:2: the two Cb and two Cr
// samples are single stores (planar or interleaved: the step decides); 4:4:4: four samples a row, through store_row4 when planar.
// Widths that are no multiple of 4 leave a tail of n = 1, 2 or 3 columns (odd only without horizontal subsampling).
template <typename T, int SUB_X, int SUB_Y, bool GREY>
__global__ __launch_bounds__(256) void planes_to_yuv420_kernel(const float* __restrict__ src, int Hs, int Ws, T* __restrict__ yp,
                                                               long long y_pitch, long long y_bstride, T* __restrict__ cbp,
                                                               T* __restrict__ crp, long long c_pitch, int c_step, long long c_bstride,
                                                               int w_out, HatCsc k, HatSample<T> q) {
    constexpr int R = 1 + SUB_Y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y * R, b = blockIdx.z;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* s = src + (size_t)b * 3 * plane + (size_t)y * Ws + x;
    const int n = min(4, w_out - x);
    float cb[R][4], cr[R][4];
    unsigned v[R][4];
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float Y = 0.f;
            cb[j][i] = cr[j][i] = 0.f;
            if (i < n) hat_rgb_to_ycc(k, s[(size_t)j * Ws + i], s[plane + (size_t)j * Ws + i], s[2 * plane + (size_t)j * Ws + i], Y, cb[j][i], cr[j][i]);
            v[j][i] = q.luma(Y);
        }
#pragma unroll
    for (int j = 0; j < R; ++j)
        store_row4(&sample_at(yp, (size_t)b * y_bstride + (size_t)(y + j) * y_pitch + (size_t)x * sizeof(T)), v[j], n);
    if constexpr (!GREY) {
        const size_t co = (size_t)b * c_bstride + (size_t)(y >> SUB_Y) * c_pitch + (size_t)(x >> SUB_X) * c_step;
        if constexpr (SUB_X == 1 && SUB_Y == 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * i < n) {
                    sample_at(cbp, co + (size_t)i * c_step) = (T)q.chroma(hat_add_rn(cb[0][2 * i], cb[0][2 * i + 1]), hat_add_rn(cb[1][2 * i], cb[1][2 * i + 1]), k.m[7]);
                    sample_at(crp, co + (size_t)i * c_step) = (T)q.chroma(hat_add_rn(cr[0][2 * i], cr[0][2 * i + 1]), hat_add_rn(cr[1][2 * i], cr[1][2 * i + 1]), k.m[11]);
                }
            }
        } else if constexpr (SUB_X == 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * i < n) {
                    sample_at(cbp, co + (size_t)i * c_step) = (T)q.luma(hat_chroma_value_h(hat_add_rn(cb[0][2 * i], cb[0][2 * i + 1]), k.m[7]));
                    sample_at(crp, co + (size_t)i * c_step) = (T)q.luma(hat_chroma_value_h(hat_add_rn(cr[0][2 * i], cr[0][2 * i + 1]), k.m[11]));
                }
            }
        } else {
            unsigned vb[4], vr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                vb[i] = q.luma(hat_add_rn(cb[0][i], k.m[7]));
                vr[i] = q.luma(hat_add_rn(cr[0][i], k.m[11]));
            }
            if (c_step == (int)sizeof(T)) {
                store_row4(&sample_at(cbp, co), vb, n);
                store_row4(&sample_at(crp, co), vr, n);
            } else {
                for (int i = 0; i < n; ++i) {
                    sample_at(cbp, co + (size_t)i * c_step) = (T)vb[i];
                    sample_at(crp, co + (size_t)i * c_step) = (T)vr[i];
                }
            }
        }
    }
}

// The same thread shape for co-sited chroma out (SUB_X = 1 always; SITING as in yuv_to_planes_sited_kernel).  The thread keeps
// its (1 + SUB_Y) x 4 tile and its Y stores, and loads column max(x - 1, 0) of its rows besides: the left tap of its first chroma
// column (the first thread of a row replicates its own column 0).  SITING 2 also loads row max(y - 1, 0), columns x - 1 .. x + 3,
// for the row tap above (the first row replicates itself).  Nothing right of x + n - 1 or below the tile is read: n is even
// here (w_out is), so column 2 i + 1 of a chroma sample that exists is inside the crop.
template <typename T, int SUB_Y, int SITING>
__global__ __launch_bounds__(256) void planes_to_yuv_sited_kernel(const float* __restrict__ src, int Hs, int Ws, T* __restrict__ yp,
                                                                  long long y_pitch, long long y_bstride, T* __restrict__ cbp,
                                                                  T* __restrict__ crp, long long c_pitch, int c_step, long long c_bstride,
                                                                  int w_out, HatCsc k, HatSample<T> q) {
    static_assert(SITING == 1 || (SITING == 2 && SUB_Y == 1), "a co-sited row axis needs vertical subsampling");
    constexpr int R = 1 + SUB_Y, UP = SITING == 2 ? 1 : 0;   // rows of the tile; rows above it (kept at index 0 of the arrays)
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y * R, b = blockIdx.z;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* s = src + (size_t)b * 3 * plane;
    const int n = min(4, w_out - x);
    // cb / cr [row][column]: row UP + j is tile row j (row 0 with UP: image row max(y - 1, 0)); column 0 is image column
    // max(x - 1, 0), column 1 + i is x + i
    float cb[UP + R][5], cr[UP + R][5];
    unsigned v[R][4];
#pragma unroll
    for (int j = 0; j < UP + R; ++j) {
        const int row = max(y + j - UP, 0);
        const float* sr = s + (size_t)row * Ws;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int col = max(x + i - 1, 0);
            float Y = 0.f;
            cb[j][i] = cr[j][i] = 0.f;
            if (i - 1 < n) hat_rgb_to_ycc(k, sr[col], sr[plane + col], sr[2 * plane + col], Y, cb[j][i], cr[j][i]);
            if (j >= UP && i >= 1) v[j - UP][i - 1] = q.luma(Y);
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j)
        store_row4(&sample_at(yp, (size_t)b * y_bstride + (size_t)(y + j) * y_pitch + (size_t)x * sizeof(T)), v[j], n);
    const size_t co = (size_t)b * c_bstride + (size_t)(y >> SUB_Y) * c_pitch + (size_t)(x >> 1) * c_step;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (2 * i < n) {
            float tb[UP + R], tr[UP + R];   // the row taps of chroma column x / 2 + i: columns 2 i - 1, 2 i, 2 i + 1 of the tile
#pragma unroll
            for (int j = 0; j < UP + R; ++j) {
                tb[j] = hat_chroma_tap121(cb[j][2 * i], cb[j][2 * i + 1], cb[j][2 * i + 2]);
                tr[j] = hat_chroma_tap121(cr[j][2 * i], cr[j][2 * i + 1], cr[j][2 * i + 2]);
            }
            float vb, vr;
            if constexpr (SUB_Y == 0) {
                vb = hat_chroma_value_s(tb[0], 0.25f, k.m[7]);
                vr = hat_chroma_value_s(tr[0], 0.25f, k.m[11]);
            } else if constexpr (SITING == 1) {
                vb = hat_chroma_value_s(hat_add_rn(tb[0], tb[1]), 0.125f, k.m[7]);
                vr = hat_chroma_value_s(hat_add_rn(tr[0], tr[1]), 0.125f, k.m[11]);
            } else {
                vb = hat_chroma_value_s(hat_chroma_tap121(tb[0], tb[1], tb[2]), 0.0625f, k.m[7]);
                vr = hat_chroma_value_s(hat_chroma_tap121(tr[0], tr[1], tr[2]), 0.0625f, k.m[11]);
            }
            sample_at(cbp, co + (size_t)i * c_step) = (T)q.luma(vb);
            sample_at(crp, co + (size_t)i * c_step) = (T)q.luma(vr);
        }
    }
}

bool even_ptrs(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 1) == 0;
}

// every entry: one launch, the instance chosen by the surface's subsampling (grey: no chroma pointers)
template <typename T, int SX, int SY, bool GREY>
void launch_to_planes(const HatYuvSurface& s, float* dst, int B, int h, int w, int Hp, int Wp, const HatCsc& k, HatSample<T> q, hipStream_t st) {
    HAT_LAUNCH((yuv420_to_planes_kernel<T, SX, SY, GREY>), dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, st, reinterpret_cast<const T*>(s.y),
               (long long)s.y_pitch, (long long)s.y_bstride, reinterpret_cast<const T*>(s.cb), reinterpret_cast<const T*>(s.cr),
               (long long)s.c_pitch, (int)s.c_step, (long long)s.c_bstride, dst, h, w, Hp, Wp, k, q);
}

template <typename T, int SX, int SY, bool GREY>
void launch_from_planes(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int h_out, int w_out, const HatCsc& k, HatSample<T> q,
                        hipStream_t st) {
    HAT_LAUNCH((planes_to_yuv420_kernel<T, SX, SY, GREY>), dim3((w_out + 1023) / 1024, h_out >> SY, B), dim3(256), 0, st, src, Hs, Ws,
               reinterpret_cast<T*>(s.y), (long long)s.y_pitch, (long long)s.y_bstride, reinterpret_cast<T*>(s.cb), reinterpret_cast<T*>(s.cr),
               (long long)s.c_pitch, (int)s.c_step, (long long)s.c_bstride, w_out, k, q);
}

template <typename T>
void surface_to_planes(const HatYuvSurface& s, float* dst, int B, int h, int w, int Hp, int Wp, const HatCsc& k, HatSample<T> q, hipStream_t st) {
    if (!s.cb) launch_to_planes<T, 0, 0, true>(s, dst, B, h, w, Hp, Wp, k, q, st);
    else if (s.sub_y) launch_to_planes<T, 1, 1, false>(s, dst, B, h, w, Hp, Wp, k, q, st);
    else if (s.sub_x) launch_to_planes<T, 1, 0, false>(s, dst, B, h, w, Hp, Wp, k, q, st);
    else launch_to_planes<T, 0, 0, false>(s, dst, B, h, w, Hp, Wp, k, q, st);
}

template <typename T>
void surface_from_planes(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int h_out, int w_out, const HatCsc& k, HatSample<T> q,
                         hipStream_t st) {
    if (!s.cb) launch_from_planes<T, 0, 0, true>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
    else if (s.sub_y) launch_from_planes<T, 1, 1, false>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
    else if (s.sub_x) launch_from_planes<T, 1, 0, false>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
    else launch_from_planes<T, 0, 0, false>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
}

// what every to-planes / from-planes entry ends in once its own checks have passed: the instance by the surface's depth
int to_planes(const HatYuvSurface& s, float* dst, int B, int h, int w, int Hp, int Wp, const float* to_rgb12, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (s.depth == 8) surface_to_planes<uint8_t>(s, dst, B, h, w, Hp, Wp, load_csc(to_rgb12), HatSample<uint8_t>{}, st);
    else surface_to_planes<uint16_t>(s, dst, B, h, w, Hp, Wp, load_csc(to_rgb12), deep_sample(s.depth, s.msb), st);
    return hat_check_launch();
}

int from_planes(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int h_out, int w_out, const float* from_rgb12, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (s.depth == 8) surface_from_planes<uint8_t>(src, B, Hs, Ws, s, h_out, w_out, load_csc(from_rgb12), HatSample<uint8_t>{}, st);
    else surface_from_planes<uint16_t>(src, B, Hs, Ws, s, h_out, w_out, load_csc(from_rgb12), deep_sample(s.depth, s.msb), st);
    return hat_check_launch();
}

// The co-sited instances.  eff: 1 ('left': x co-sited) or 2 ('topleft': x and y), what hat_siting_of makes of a siting and a surface.
template <typename T, int SY, int SITING>
void launch_to_planes_sited(const HatYuvSurface& s, float* dst, int B, int h, int w, int Hp, int Wp, const HatCsc& k, HatSample<T> q, hipStream_t st) {
    HAT_LAUNCH((yuv_to_planes_sited_kernel<T, SY, SITING>), dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, st, reinterpret_cast<const T*>(s.y),
               (long long)s.y_pitch, (long long)s.y_bstride, reinterpret_cast<const T*>(s.cb), reinterpret_cast<const T*>(s.cr),
               (long long)s.c_pitch, (int)s.c_step, (long long)s.c_bstride, dst, h, w, Hp, Wp, k, q);
}

template <typename T, int SY, int SITING>
void launch_from_planes_sited(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int h_out, int w_out, const HatCsc& k,
                              HatSample<T> q, hipStream_t st) {
    HAT_LAUNCH((planes_to_yuv_sited_kernel<T, SY, SITING>), dim3((w_out + 1023) / 1024, h_out >> SY, B), dim3(256), 0, st, src, Hs, Ws,
               reinterpret_cast<T*>(s.y), (long long)s.y_pitch, (long long)s.y_bstride, reinterpret_cast<T*>(s.cb), reinterpret_cast<T*>(s.cr),
               (long long)s.c_pitch, (int)s.c_step, (long long)s.c_bstride, w_out, k, q);
}

template <typename T>
void surface_to_planes_sited(const HatYuvSurface& s, int eff, float* dst, int B, int h, int w, int Hp, int Wp, const HatCsc& k, HatSample<T> q,
                             hipStream_t st) {
    if (!s.sub_y) launch_to_planes_sited<T, 0, 1>(s, dst, B, h, w, Hp, Wp, k, q, st);
    else if (eff == 1) launch_to_planes_sited<T, 1, 1>(s, dst, B, h, w, Hp, Wp, k, q, st);
    else launch_to_planes_sited<T, 1, 2>(s, dst, B, h, w, Hp, Wp, k, q, st);
}

template <typename T>
void surface_from_planes_sited(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int eff, int h_out, int w_out, const HatCsc& k,
                               HatSample<T> q, hipStream_t st) {
    if (!s.sub_y) launch_from_planes_sited<T, 0, 1>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
    else if (eff == 1) launch_from_planes_sited<T, 1, 1>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
    else launch_from_planes_sited<T, 1, 2>(src, B, Hs, Ws, s, h_out, w_out, k, q, st);
}

// the padded planes hold the frame, fit the grid, and the reflection has a source row / column: pad < size
bool padded_ok(int B, int h, int w, int Hp, int Wp) { return Hp >= h && Wp >= w && B <= 65535 && Hp <= 65535 && Hp - h < h && Wp - w < w; }

}  // namespace

extern "C" int hat_yuv_to_planes(const HatYuvSurface* src, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp, int32_t Wp,
                                 const float* to_rgb12, void* stream) {
    if (!dst || !to_rgb12 || !hat_yuv_surface_ok(src, B, h, w) || !padded_ok(B, h, w, Hp, Wp)) return HAT_EINVAL;
    return to_planes(*src, dst, B, h, w, Hp, Wp, to_rgb12, stream);
}

extern "C" int hat_planes_to_yuv(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatYuvSurface* dst, int32_t h_out, int32_t w_out,
                                 const float* from_rgb12, void* stream) {
    if (!src || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out > 65535) return HAT_EINVAL;
    return from_planes(src, B, Hs, Ws, *dst, h_out, w_out, from_rgb12, stream);
}

// The sited entries: the unsited entries' checks, then the siting.  What the surface makes centre of it (siting 0, 4:4:4, grey)
// IS the unsited entry; the rest launches a co-sited instance on the same grid.
extern "C" int hat_yuv_to_planes_sited(const HatYuvSurface* src, int32_t siting, float* dst, int32_t B, int32_t h, int32_t w, int32_t Hp,
                                       int32_t Wp, const float* to_rgb12, void* stream) {
    if (!hat_siting_ok(siting) || !dst || !to_rgb12 || !hat_yuv_surface_ok(src, B, h, w) || !padded_ok(B, h, w, Hp, Wp)) return HAT_EINVAL;
    const int eff = hat_siting_of(src, siting);
    if (eff == HAT_SITING_CENTER) return hat_yuv_to_planes(src, dst, B, h, w, Hp, Wp, to_rgb12, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (src->depth == 8) surface_to_planes_sited<uint8_t>(*src, eff, dst, B, h, w, Hp, Wp, load_csc(to_rgb12), HatSample<uint8_t>{}, st);
    else surface_to_planes_sited<uint16_t>(*src, eff, dst, B, h, w, Hp, Wp, load_csc(to_rgb12), deep_sample(src->depth, src->msb), st);
    return hat_check_launch();
}

extern "C" int hat_planes_to_yuv_sited(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatYuvSurface* dst, int32_t siting,
                                       int32_t h_out, int32_t w_out, const float* from_rgb12, void* stream) {
    if (!hat_siting_ok(siting) || !src || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out > 65535) return HAT_EINVAL;
    const int eff = hat_siting_of(dst, siting);
    if (eff == HAT_SITING_CENTER) return hat_planes_to_yuv(src, B, Hs, Ws, dst, h_out, w_out, from_rgb12, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dst->depth == 8) surface_from_planes_sited<uint8_t>(src, B, Hs, Ws, *dst, eff, h_out, w_out, load_csc(from_rgb12), HatSample<uint8_t>{}, st);
    else surface_from_planes_sited<uint16_t>(src, B, Hs, Ws, *dst, eff, h_out, w_out, load_csc(from_rgb12), deep_sample(dst->depth, dst->msb), st);
    return hat_check_launch();
}

// The 4:2:0 entries: their own argument lists and checks, then the (1,1) surface of their block through the same two functions
// (the grid of a 4:2:0 from-planes launch has h_out / 2 rows, so these two take frames twice as tall as hat_planes_to_yuv does).
extern "C" int hat_yuv420_to_planes(const uint8_t* y, int64_t y_pitch, int64_t y_bstride, const uint8_t* cb, const uint8_t* cr,
                                    int64_t c_pitch, int32_t c_step, int64_t c_bstride, float* dst, int32_t B, int32_t h, int32_t w,
                                    int32_t Hp, int32_t Wp, const float* to_rgb12, void* stream) {
    if (!y || !cb || !cr || !dst || !to_rgb12 || !hat_yuv_block_ok(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h, w)) return HAT_EINVAL;
    if (!padded_ok(B, h, w, Hp, Wp)) return HAT_EINVAL;
    return to_planes(hat_yuv420_surface(y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride, 8, 0), dst, B, h, w, Hp, Wp, to_rgb12, stream);
}

extern "C" int hat_planes_to_yuv420(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint8_t* y, int64_t y_pitch, int64_t y_bstride,
                                    uint8_t* cb, uint8_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t h_out,
                                    int32_t w_out, const float* from_rgb12, void* stream) {
    if (!src || !y || !cb || !cr || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_block_ok(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h_out, w_out))
        return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out / 2 > 65535) return HAT_EINVAL;
    return from_planes(src, B, Hs, Ws, hat_yuv420_surface(y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride, 8, 0), h_out, w_out, from_rgb12, stream);
}

// The deep forms: the same on 16-bit words.  Pitches, strides and c_step are in bytes and even.
extern "C" int hat_yuv420p16_to_planes(const uint16_t* y, int64_t y_pitch, int64_t y_bstride, const uint16_t* cb, const uint16_t* cr,
                                       int64_t c_pitch, int32_t c_step, int64_t c_bstride, float* dst, int32_t B, int32_t h, int32_t w,
                                       int32_t Hp, int32_t Wp, const float* to_rgb12, int32_t depth, int32_t msb, void* stream) {
    if (!y || !cb || !cr || !dst || !to_rgb12 || !hat_yuv_depth_ok(depth, msb) || !even_ptrs(y, cb, cr) ||
        !hat_yuv_block_ok_n(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h, w, 2))
        return HAT_EINVAL;
    if (!padded_ok(B, h, w, Hp, Wp)) return HAT_EINVAL;
    return to_planes(hat_yuv420_surface(y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride, depth, msb), dst, B, h, w, Hp, Wp, to_rgb12, stream);
}

extern "C" int hat_planes_to_yuv420p16(const float* src, int32_t B, int32_t Hs, int32_t Ws, uint16_t* y, int64_t y_pitch, int64_t y_bstride,
                                       uint16_t* cb, uint16_t* cr, int64_t c_pitch, int32_t c_step, int64_t c_bstride, int32_t h_out,
                                       int32_t w_out, const float* from_rgb12, int32_t depth, int32_t msb, void* stream) {
    if (!src || !y || !cb || !cr || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_depth_ok(depth, msb) || !even_ptrs(y, cb, cr) ||
        !hat_yuv_block_ok_n(y_pitch, y_bstride, c_pitch, c_step, c_bstride, B, h_out, w_out, 2))
        return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out / 2 > 65535) return HAT_EINVAL;
    return from_planes(src, B, Hs, Ws, hat_yuv420_surface(y, y_pitch, y_bstride, cb, cr, c_pitch, c_step, c_bstride, depth, msb), h_out, w_out, from_rgb12, stream);
}
