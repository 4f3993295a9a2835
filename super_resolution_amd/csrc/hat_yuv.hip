// hat_yuv.hip — the 4:2:0 frame boundary: YCbCr frames (NV12 / NV21 / I420, bytes; P010 / P012 / P016 / yuv420p1xle, 16-bit
// words) <-> the network's fp32 RGB planes.  Contract: include/hat_mi355x.h (hat_yuv420_to_planes, hat_planes_to_yuv420 and
// their p16 forms); definition: super_resolution_amd/yuv.py;
// colour conversion: basicsr utils/color_util.py (rgb2ycbcr, ycbcr2rgb: BT.601, 16-235), shared with conv_last's yuv epilogue
// through hat_common.h (hat_ycc_to_rgb, hat_rgb_to_ycc).  cb and cr are separate pointers with a byte step between the
// samples of a row (1: planar, 2: interleaved), so one kernel serves all three layouts.  The chroma subsampling (SUB_X, SUB_Y) and
// grey (no chroma) are template parameters of the same two kernels: (1,1) is 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4; the surface
// entries (hat_yuv_to_planes, hat_planes_to_yuv) pick the instance.  Those are centre-sited chroma (nearest up, box down); the
// co-sited instances ('left', 'topleft': hat_yuv_to_planes_sited, hat_planes_to_yuv_sited) are kernels of their own beside them.
#include "hat_frame_sink.h"

namespace {

// one thread = one pixel of the padded plane row (hat_u8_to_planes' shape): a Y sample, the Cb and Cr samples of its 2 x 2 block
// (the four pixels of a block read the same two samples: L1), three plane stores coalesced over the lanes.  Reflection as in
// u8_to_planes_kernel; the chroma sample of source pixel (sy, sx) is (sy >> SUB_Y, sx >> SUB_X).  GREY: no chroma is read, both
// samples are the neutral one.
template <typename T, int SUB_X, int SUB_Y, bool GREY>
__global__ __launch_bounds__(256) void yuv420_to_planes_kernel(const HatYuvDst<const T> s, float* __restrict__ dst, int h, int w, int Hp, int Wp,
                                                               HatCsc k, HatSample<T> q) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    float rgb[3];
    const unsigned Yw = s.luma(b, sy, sx);
    if constexpr (GREY) {
        q.to_rgb(k, Yw, q.neutral(), q.neutral(), rgb);
    } else {
        const size_t co = s.chroma(b, sy >> SUB_Y, sx >> SUB_X);
        q.to_rgb(k, Yw, sample_at(s.cb, co), sample_at(s.cr, co), rgb);
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
__global__ __launch_bounds__(256) void yuv_to_planes_sited_kernel(const HatYuvDst<const T> s, float* __restrict__ dst, int h, int w, int Hp,
                                                                  int Wp, HatCsc k, HatSample<T> q) {
    static_assert(SITING == 1 || (SITING == 2 && SUB_Y == 1), "a co-sited row axis needs vertical subsampling");
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wp) return;
    const int sy = y < h ? y : 2 * (h - 1) - y, sx = x < w ? x : 2 * (w - 1) - x;
    const int cw = w >> 1, ch = h >> SUB_Y;
    const int j = sx >> 1, j1 = min(j + (sx & 1), cw - 1);
    const int i = sy >> SUB_Y, i1 = SITING == 2 ? min(i + (sy & 1), ch - 1) : i;
    const float Y = q.value(s.luma(b, sy, sx));
    const size_t c00 = s.chroma(b, i, j), c01 = s.chroma(b, i, j1), c10 = s.chroma(b, i1, j), c11 = s.chroma(b, i1, j1);
    const float cb = hat_chroma_up4(q.value(sample_at(s.cb, c00)), q.value(sample_at(s.cb, c01)), q.value(sample_at(s.cb, c10)), q.value(sample_at(s.cb, c11)));
    const float cr = hat_chroma_up4(q.value(sample_at(s.cr, c00)), q.value(sample_at(s.cr, c01)), q.value(sample_at(s.cr, c10)), q.value(sample_at(s.cr, c11)));
    float rgb[3];
    hat_ycc_to_rgb_f(k, Y, cb, cr, rgb);
    float* o = dst + ((size_t)b * 3 * Hp + y) * Wp + x;
    const size_t plane = (size_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = rgb[c];
}

// one thread = (1 + SUB_Y) rows x four columns: per row and plane 16 contiguous bytes are loaded, and yuv_store_tile
// (hat_frame_sink.h) converts and stores them.  Widths that are no multiple of 4 leave a tail of n = 1, 2 or 3 columns.
template <typename T, int SUB_X, int SUB_Y, bool GREY>
__global__ __launch_bounds__(256) void planes_to_yuv420_kernel(const float* __restrict__ src, int Hs, int Ws, const HatYuvDst<T> d, int w_out,
                                                               HatCsc k, HatSample<T> q) {
    constexpr int R = 1 + SUB_Y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y * R, b = blockIdx.z;
    if (x >= w_out) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* s = src + (size_t)b * 3 * plane + (size_t)y * Ws + x;
    const int n = min(4, w_out - x);
    yuv_store_tile<T, SUB_X, SUB_Y, GREY>(d, k, q, b, y, x, n, [&](float (&rgb)[R][4][3]) {
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[j][i][c] = i < n ? s[c * plane + (size_t)j * Ws + i] : 0.f;
    });
}

// The same thread shape for co-sited chroma out (SUB_X = 1 always; SITING as in yuv_to_planes_sited_kernel).  The thread keeps
// its (1 + SUB_Y) x 4 tile and its Y stores, and loads column max(x - 1, 0) of its rows besides: the left tap of its first chroma
// column (the first thread of a row replicates its own column 0).  SITING 2 also loads row max(y - 1, 0), columns x - 1 .. x + 3,
// for the row tap above (the first row replicates itself).  Nothing right of x + n - 1 or below the tile is read: n is even
// here (w_out is), so column 2 i + 1 of a chroma sample that exists is inside the crop.
template <typename T, int SUB_Y, int SITING>
__global__ __launch_bounds__(256) void planes_to_yuv_sited_kernel(const float* __restrict__ src, int Hs, int Ws, const HatYuvDst<T> d, int w_out,
                                                                  HatCsc k, HatSample<T> q) {
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
    for (int j = 0; j < R; ++j) store_row4(&d.luma(b, y + j, x), v[j], n);
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
            const size_t co = d.chroma(b, y >> SUB_Y, (x >> 1) + i);
            sample_at(d.cb, co) = (T)q.luma(vb);
            sample_at(d.cr, co) = (T)q.luma(vr);
        }
    }
}

bool even_ptrs(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 1) == 0;
}

// what every to-planes / from-planes entry ends in once its own checks have passed: one launch, the instance by the surface
// (yuv_dispatch)
int to_planes(const HatYuvSurface& s, float* dst, int B, int h, int w, int Hp, int Wp, const float* to_rgb12, void* stream) {
    yuv_dispatch(s, [&](auto L, auto q) {
        using T = typename decltype(L)::sample_t;
        HAT_LAUNCH((yuv420_to_planes_kernel<T, L.sx, L.sy, L.grey>), dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                   yuv_dst<const T>(s), dst, h, w, Hp, Wp, load_csc(to_rgb12), q);
    });
    return hat_check_launch();
}

int from_planes(const float* src, int B, int Hs, int Ws, const HatYuvSurface& s, int h_out, int w_out, const float* from_rgb12, void* stream) {
    yuv_dispatch(s, [&](auto L, auto q) {
        using T = typename decltype(L)::sample_t;
        HAT_LAUNCH((planes_to_yuv420_kernel<T, L.sx, L.sy, L.grey>), dim3((w_out + 1023) / 1024, h_out >> L.sy, B), dim3(256), 0,
                   reinterpret_cast<hipStream_t>(stream), src, Hs, Ws, yuv_dst<T>(s), w_out, load_csc(from_rgb12), q);
    });
    return hat_check_launch();
}

// The co-sited instances, chosen on other keys: f(SY, SITING as integral constants) by the surface's sub_y and by eff, 1 ('left': x
// co-sited) or 2 ('topleft': x and y), what hat_siting_of makes of a siting and a surface.
template <typename F> void sited_dispatch(const HatYuvSurface& s, int eff, F&& f) {
    if (!s.sub_y) f(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    else if (eff == 1) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
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
    yuv_dispatch_depth(*src, [&](auto q) {
        using T = typename decltype(q)::sample_t;
        sited_dispatch(*src, eff, [&](auto sy, auto siting) {
            HAT_LAUNCH((yuv_to_planes_sited_kernel<T, sy(), siting()>), dim3((Wp + 255) / 256, Hp, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       yuv_dst<const T>(*src), dst, h, w, Hp, Wp, load_csc(to_rgb12), q);
        });
    });
    return hat_check_launch();
}

extern "C" int hat_planes_to_yuv_sited(const float* src, int32_t B, int32_t Hs, int32_t Ws, const HatYuvSurface* dst, int32_t siting,
                                       int32_t h_out, int32_t w_out, const float* from_rgb12, void* stream) {
    if (!hat_siting_ok(siting) || !src || !from_rgb12 || Hs < 1 || Ws < 1 || !hat_yuv_surface_ok(dst, B, h_out, w_out)) return HAT_EINVAL;
    if (h_out > Hs || w_out > Ws || B > 65535 || h_out > 65535) return HAT_EINVAL;
    const int eff = hat_siting_of(dst, siting);
    if (eff == HAT_SITING_CENTER) return hat_planes_to_yuv(src, B, Hs, Ws, dst, h_out, w_out, from_rgb12, stream);
    yuv_dispatch_depth(*dst, [&](auto q) {
        using T = typename decltype(q)::sample_t;
        sited_dispatch(*dst, eff, [&](auto sy, auto siting) {
            HAT_LAUNCH((planes_to_yuv_sited_kernel<T, sy(), siting()>), dim3((w_out + 1023) / 1024, h_out >> sy(), B), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, Hs, Ws, yuv_dst<T>(*dst), w_out, load_csc(from_rgb12), q);
        });
    });
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
