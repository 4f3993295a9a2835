// hat_plan.cpp — whole-network entry points for hosts without Python (contract: "Forward plans" in include/hat_mi355x.h).
//
// A plan is the complete launch list of one HAT forward for one input shape — every C-ABI call of this library in order,
// with its descriptors / scalars and with every device pointer expressed as (buffer id, byte offset) — plus the buffers
// themselves: packed weights and constants (with their bytes), workspace (zero-initialised), the input and the output.
// `python -m super_resolution_amd.plan` writes it (it records the calls the Python engine makes for that shape, so whatever
// the engine does — fused or unfused kernels, any model variant — is what the plan replays); hat_plan_load() allocates and
// uploads, hat_plan_forward() patches the pointers and issues the same kernels on ONE stream.  No Python, no torch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stddef.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/hat_mi355x.h"
#include "hat_packed_check.h"
#include "hat_plan_parse.h"
#include "hat_yuv_check.h"

// the file format's types, the function table and the parser: host-only code, shared with hat_plan_check.cpp
using namespace hat_plan_host;

struct hat_plan {
    int32_t dims[8];   // B, Cin, H, W, scale, Cout, dtype, reserved
    std::vector<Buf> bufs;
    std::vector<Call> calls;
    int device = -1;   // the device the buffers were allocated on (hat_plan_forward refuses to launch on another one)
    // hat_plan_forward_u8's fp32 staging (allocated by its first call, freed with the plan; `mutable`: the C API hands plans
    // out as const, and like the workspace these belong to the one forward that may run at a time)
    mutable float* stage_in = nullptr;
    mutable float* stage_out = nullptr;
};

namespace {

struct Resolved {   // argument values of one call with the pointers patched
    const hat_plan* p;
    const Call* c;
    const void* x;
    void* y;
    void* stream;
    std::vector<std::vector<unsigned char>> tmp;
    void* ptr(uint32_t buf, uint64_t off) const {
        if (buf == NULL_BUF) return nullptr;
        const Buf& b = p->bufs[buf];
        char* base = b.kind == BUF_INPUT ? (char*)const_cast<void*>(x) : (b.kind == BUF_OUTPUT ? (char*)y : (char*)b.dev);
        return base + off;
    }
    int32_t I(size_t k) const { return (int32_t)c->args[k].i; }
    int64_t L(size_t k) const { return c->args[k].i; }
    float F(size_t k) const { return (float)c->args[k].f; }
    void* P(size_t k) {
        const Arg& a = c->args[k];
        if (a.tag == ARG_PTR) return ptr(a.buf, a.off);
        if (a.tag == ARG_STREAM) return stream;
        if (a.tag == ARG_STRUCT || a.tag == ARG_HOST) {
            tmp.emplace_back(a.blob);
            for (const Fix& fx : a.fix) {
                void* v = ptr(fx.buf, fx.off);
                memcpy(tmp.back().data() + fx.field_off, &v, sizeof(void*));
            }
            return tmp.back().data();
        }
        return nullptr;
    }
};

// One recorded call -> the entry point's own parameter list, position by position and by the parameter's C type: the rule
// hat_plan_parse.h builds SIGNATURES by, so what the parser accepted is exactly what is read here (int32_t: I, int64_t: L,
// float: F, any pointer — device pointer, descriptor, host array or the stream — P).
template <class T> T arg_as(Resolved& r, size_t k) {
    if constexpr (std::is_same_v<T, int32_t>) return r.I(k);
    else if constexpr (std::is_same_v<T, int64_t>) return r.L(k);
    else if constexpr (std::is_same_v<T, float>) return r.F(k);
    else return (T)r.P(k);
}
template <class... A, size_t... K> int replay(int (*fn)(A...), Resolved& r, std::index_sequence<K...>) { return fn(arg_as<A>(r, K)...); }
template <class... A> int replay(int (*fn)(A...), Resolved& r) {
    return r.c->args.size() == sizeof...(A) ? replay(fn, r, std::index_sequence_for<A...>{}) : HAT_EINVAL;
}

int dispatch(Resolved& r) {
    switch (r.c->fn) {
#define HAT_PLAN_CASE(f) case FN_##f: return replay(&f, r);
        HAT_PLAN_FUNCTIONS(HAT_PLAN_CASE)
#undef HAT_PLAN_CASE
        default: return HAT_EUNSUPPORTED;
    }
}

}  // namespace

extern "C" void hat_plan_free(hat_plan* p) {
    if (!p) return;
    for (Buf& b : p->bufs)
        if (b.dev) (void)hipFree(b.dev);
    if (p->stage_in) (void)hipFree(p->stage_in);
    if (p->stage_out) (void)hipFree(p->stage_out);
    delete p;
}

static int plan_load_impl(const char* path, hat_plan** out);

// The file is untrusted input.  hat_plan_parse (hat_plan_parse.h: host code, the rules are listed there) reads and checks ALL of
// it first; only a file that passed allocates.  Nothing thrown by the containers may cross the extern "C" boundary.
extern "C" int hat_plan_load(const char* path, hat_plan** out) {
    if (!path || !out) return HAT_EINVAL;
    *out = nullptr;
    try {
        return plan_load_impl(path, out);
    } catch (...) {
        return HAT_EINVAL;
    }
}

namespace {
struct PlanGuard {   // frees a half-built plan on every exit path, exceptions included
    hat_plan* p;
    ~PlanGuard() { if (p) hat_plan_free(p); }
};
}  // namespace

static int plan_load_impl(const char* path, hat_plan** out) {
    FILE* f = fopen(path, "rb");
    if (!f) return HAT_EINVAL;
    struct FileGuard { FILE* f; ~FileGuard() { fclose(f); } } fguard{f};
    hat_plan* p = new hat_plan();
    PlanGuard guard{p};
    {
        Parsed parsed;
        if (const int rc = hat_plan_parse(f, &parsed)) return rc;   // refused: no device call has been made
        memcpy(p->dims, parsed.dims, sizeof(p->dims));
        p->bufs = std::move(parsed.bufs);     // every dev is still null: from here on the guard frees what the loop below allocates,
        p->calls = std::move(parsed.calls);   // because each hipMalloc writes straight into the plan's own entry
    }
    if (hipGetDevice(&p->device) != hipSuccess) return HAT_EINVAL;
    std::vector<unsigned char> host;
    for (Buf& b : p->bufs) {
        if (b.kind != BUF_CONST && b.kind != BUF_SCRATCH) continue;
        hipError_t e = hipMalloc(&b.dev, b.nbytes ? b.nbytes : 16);
        if (e != hipSuccess) { b.dev = nullptr; return (int)e; }
        if (b.kind == BUF_CONST) {
            host.resize(b.nbytes);
            if (fseeko(f, (off_t)b.file_off, SEEK_SET) != 0 || (b.nbytes && fread(host.data(), 1, b.nbytes, f) != b.nbytes)) return HAT_EINVAL;
            e = hipMemcpy(b.dev, host.data(), b.nbytes, hipMemcpyHostToDevice);
        } else {
            e = hipMemset(b.dev, 0, b.nbytes ? b.nbytes : 16);
        }
        if (e != hipSuccess) return (int)e;
    }
    if (const hipError_t e = hipDeviceSynchronize()) return (int)e;
    guard.p = nullptr;       // (on every return above the guards free the plan and close the file)
    *out = p;
    return 0;
}

extern "C" int hat_plan_info(const hat_plan* p, int32_t* dims8, int64_t* n_calls, int64_t* device_bytes) {
    if (!p) return HAT_EINVAL;
    if (dims8) memcpy(dims8, p->dims, sizeof(p->dims));
    if (n_calls) *n_calls = (int64_t)p->calls.size();
    if (device_bytes) {
        int64_t s = 0;
        for (const Buf& b : p->bufs)
            if (b.dev) s += (int64_t)b.nbytes;
        *device_bytes = s;
    }
    return 0;
}

extern "C" int hat_plan_forward(const hat_plan* p, const float* x, float* y, void* stream) {
    if (!p || !x || !y) return HAT_EINVAL;
    int dev = -1;
    // the kernels launch on the CURRENT device: it must be the one the plan's buffers live on
    if (hipGetDevice(&dev) != hipSuccess || dev != p->device) return HAT_EINVAL;
    for (const Call& c : p->calls) {
        Resolved r{p, &c, x, y, stream, {}};
        const int rc = dispatch(r);
        if (rc) return rc;
    }
    return 0;
}

namespace {
bool addresses_output(const hat_plan* p, const Call& c) {
    for (const Arg& a : c.args) {
        if (a.tag == ARG_PTR && a.buf != NULL_BUF && p->bufs[a.buf].kind == BUF_OUTPUT) return true;
        for (const Fix& fx : a.fix)
            if (fx.buf != NULL_BUF && p->bufs[fx.buf].kind == BUF_OUTPUT) return true;
    }
    return false;
}

// The recorded forward ends with a launch that writes three planes to the start of the output buffer and no earlier launch
// touches that buffer: the fp32 image can be skipped (the earlier launches are then replayed without an output).  That launch is
// hat_conv3x3_to_planes (ENDS_CONV_LAST) or the folded ending, a hat_conv call whose descriptor has out_mode
// HAT_O_FOLD2_NCHW_F32 (ENDS_FOLDED: hat_upfold_to_planes behind a HatConvDesc).  ENDS_OTHER: neither.
enum Ending { ENDS_OTHER = 0, ENDS_CONV_LAST, ENDS_FOLDED };
Ending ending_of(const hat_plan* p) {
    if (p->calls.empty()) return ENDS_OTHER;
    const Call& c = p->calls.back();
    Ending e = ENDS_OTHER;
    if (c.fn == FN_hat_conv3x3_to_planes) {
        if (c.args.size() != 14 || c.args[3].tag != ARG_PTR || c.args[3].buf >= p->bufs.size()) return ENDS_OTHER;
        if (p->bufs[c.args[3].buf].kind != BUF_OUTPUT || c.args[3].off != 0 || c.args[9].i != 3) return ENDS_OTHER;
        e = ENDS_CONV_LAST;
    } else if (c.fn == FN_hat_conv) {
        if (c.args.size() != 2 || c.args[0].tag != ARG_STRUCT || c.args[0].blob.size() != sizeof(HatConvDesc)) return ENDS_OTHER;
        HatConvDesc d;
        memcpy(&d, c.args[0].blob.data(), sizeof(d));
        if (d.out_mode != HAT_O_FOLD2_NCHW_F32) return ENDS_OTHER;
        bool out_ok = false;
        for (const Fix& fx : c.args[0].fix)
            if (fx.field_off == offsetof(HatConvDesc, out))
                out_ok = fx.buf != NULL_BUF && fx.buf < p->bufs.size() && p->bufs[fx.buf].kind == BUF_OUTPUT && fx.off == 0;
        if (!out_ok) return ENDS_OTHER;
        e = ENDS_FOLDED;
    } else {
        return ENDS_OTHER;
    }
    for (size_t k = 0; k + 1 < p->calls.size(); ++k)
        if (addresses_output(p, p->calls[k])) return ENDS_OTHER;
    return e;
}

// What the frame entries share once their own checks have passed: the device check, the fp32 staging (allocated by the first
// call), source(stage_in), the replay of all but a final planes launch (ending_of), and the ending: fused(r, ending), that
// launch's sink form on the recorded arguments r of the last call, or planes(stage_out, Hs, Ws) after a replay of every call.
// may_fuse = false: the ending has no epilogue form (a co-sited YCbCr destination), so the final planes launch is replayed
// like every other call, into the output staging image.
template <typename Source, typename Fused, typename Planes>
int forward_frames(const hat_plan* p, void* stream, Source source, Fused fused_sink, Planes planes_sink, bool may_fuse = true) {
    const int32_t B = p->dims[0], H = p->dims[2], W = p->dims[3], s = p->dims[4];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != p->device) return HAT_EINVAL;
    const Ending ending = may_fuse ? ending_of(p) : ENDS_OTHER;
    const bool fused = ending != ENDS_OTHER;
    if (!p->stage_in) {
        const hipError_t e = hipMalloc((void**)&p->stage_in, (size_t)B * 3 * H * W * sizeof(float));
        if (e != hipSuccess) { p->stage_in = nullptr; return (int)e; }
    }
    if (!fused && !p->stage_out) {
        const hipError_t e = hipMalloc((void**)&p->stage_out, (size_t)B * 3 * s * H * s * W * sizeof(float));
        if (e != hipSuccess) { p->stage_out = nullptr; return (int)e; }
    }
    int rc = source(p->stage_in);
    if (rc) return rc;
    const size_t n = p->calls.size() - (fused ? 1 : 0);
    for (size_t k = 0; k < n; ++k) {
        Resolved r{p, &p->calls[k], p->stage_in, p->stage_out, stream, {}};
        rc = dispatch(r);
        if (rc) return rc;
    }
    if (!fused) return planes_sink(p->stage_out, s * H, s * W);
    Resolved r{p, &p->calls.back(), p->stage_in, nullptr, stream, {}};
    return fused_sink(r, ending);
}

// a three-channel plan whose (H, W) the (h, w) frame reflect-pads to
int frame_fits(const hat_plan* p, int32_t h, int32_t w) {
    const int32_t H = p->dims[2], W = p->dims[3];
    if (p->dims[1] != 3 || p->dims[5] != 3) return HAT_EUNSUPPORTED;   // frames become three-channel images
    return h > H || w > W || H - h >= h || W - w >= w ? HAT_EINVAL : 0;
}

// One side of a YCbCr frame forward: a planar / semi-planar surface or a packed 4:2:2 one (exactly one is set), and its siting.
struct FrameSide {
    const HatYuvSurface* planar;
    const HatPackedSurface* packed;
    int32_t siting;
    bool ok(int32_t B, int64_t h, int64_t w) const { return packed ? hat_packed_surface_ok(packed, B, h, w) : hat_yuv_surface_ok(planar, B, h, w); }
    bool centre() const { return !packed && hat_siting_of(planar, siting) == HAT_SITING_CENTER; }   // (of a checked surface)
};

// hat_plan_forward_yuv after its NULL checks.  The 4:2:0 entries come here with the (1,1) surfaces of their blocks and their own
// from-planes entry (planes420: its grid takes frames twice as tall as hat_planes_to_yuv's).  A packed side (hat_plan_forward_packed422)
// has no fused ending, like a co-sited one.
int forward_yuv(const hat_plan* p, const FrameSide& src, const FrameSide& dst, int32_t h, int32_t w, const float* to_rgb12,
                const float* from_rgb12, void* stream, bool planes420) {
    // what needs no plan first (a B of 1 stands in: the batch strides are checked against the plan's B below)
    if (!src.ok(1, h, w)) return HAT_EINVAL;
    if (const int rc = frame_fits(p, h, w)) return rc;
    const int32_t B = p->dims[0], H = p->dims[2], W = p->dims[3], s = p->dims[4], ho = s * h, wo = s * w;
    // both surfaces in full before anything is enqueued (the kernels' own checks would refuse the destination only after the replay)
    if (!src.ok(B, h, w) || !dst.ok(B, (int64_t)s * h, (int64_t)s * w)) return HAT_EINVAL;
    const bool sited_out = !dst.centre();   // (a sited or packed entry: never planes420)
    return forward_frames(
        p, stream,
        [&](float* in) {
            if (src.packed) return hat_packed422_to_planes(src.packed, src.siting, in, B, h, w, H, W, to_rgb12, stream);
            if (src.centre()) return hat_yuv_to_planes(src.planar, in, B, h, w, H, W, to_rgb12, stream);
            return hat_yuv_to_planes_sited(src.planar, src.siting, in, B, h, w, H, W, to_rgb12, stream);
        },
        [&](Resolved& r, Ending ending) {
            if (ending == ENDS_FOLDED) {
                const HatConvDesc* d = (const HatConvDesc*)r.P(0);
                return hat_upfold_to_yuv(d->x, d->w, d->bias, dst.planar, d->B, d->H, d->W, d->ldx, ho, wo, d->out_scale, d->mean[0], d->mean[1],
                                         d->mean[2], from_rgb12, d->dtype, stream);
            }
            return hat_conv3x3_to_yuv(r.P(0), r.P(1), (const float*)r.P(2), dst.planar, r.I(4), r.I(5), r.I(6), r.I(7), r.I(8), ho, wo, r.F(10),
                                      (const float*)r.P(11), from_rgb12, r.I(12), stream);
        },
        [&](const float* out, int32_t Hs, int32_t Ws) {
            if (dst.packed) return hat_planes_to_packed422(out, B, Hs, Ws, dst.packed, dst.siting, ho, wo, from_rgb12, stream);
            const HatYuvSurface& d = *dst.planar;
            if (sited_out) return hat_planes_to_yuv_sited(out, B, Hs, Ws, dst.planar, dst.siting, ho, wo, from_rgb12, stream);
            if (!planes420) return hat_planes_to_yuv(out, B, Hs, Ws, dst.planar, ho, wo, from_rgb12, stream);
            if (d.depth == 8)
                return hat_planes_to_yuv420(out, B, Hs, Ws, (uint8_t*)d.y, d.y_pitch, d.y_bstride, (uint8_t*)d.cb, (uint8_t*)d.cr, d.c_pitch, d.c_step,
                                            d.c_bstride, ho, wo, from_rgb12, stream);
            return hat_planes_to_yuv420p16(out, B, Hs, Ws, (uint16_t*)d.y, d.y_pitch, d.y_bstride, (uint16_t*)d.cb, (uint16_t*)d.cr, d.c_pitch, d.c_step,
                                           d.c_bstride, ho, wo, from_rgb12, d.depth, d.msb, stream);
        },
        !sited_out);
}

// the planar sides of the entries that know no packed surface
int forward_yuv(const hat_plan* p, const HatYuvSurface* src, const HatYuvSurface* dst, int32_t h, int32_t w, const float* to_rgb12,
                const float* from_rgb12, void* stream, bool planes420, int32_t src_siting = HAT_SITING_CENTER,
                int32_t dst_siting = HAT_SITING_CENTER) {
    return forward_yuv(p, FrameSide{src, nullptr, src_siting}, FrameSide{dst, nullptr, dst_siting}, h, w, to_rgb12, from_rgb12, stream, planes420);
}
}  // namespace

extern "C" int hat_plan_forward_u8(const hat_plan* p, const uint8_t* src, int64_t src_pitch, int32_t h, int32_t w, uint8_t* dst,
                                   int64_t dst_pitch, int32_t flags, void* stream) {
    if (!p || !src || !dst || h < 1 || w < 1 || src_pitch < 3 * (int64_t)w) return HAT_EINVAL;
    if (const int rc = frame_fits(p, h, w)) return rc;
    const int32_t B = p->dims[0], H = p->dims[2], W = p->dims[3], s = p->dims[4];
    if (dst_pitch < 3 * (int64_t)s * w) return HAT_EINVAL;
    const int bgr = flags & 1, ho = s * h, wo = s * w;
    return forward_frames(
        p, stream, [&](float* in) { return hat_u8_to_planes(src, src_pitch, src_pitch * h, in, B, h, w, H, W, bgr, stream); },
        [&](Resolved& r, Ending ending) {
            if (ending == ENDS_FOLDED) {
                const HatConvDesc* d = (const HatConvDesc*)r.P(0);
                return hat_upfold_to_u8(d->x, d->w, d->bias, dst, dst_pitch, dst_pitch * ho, d->B, d->H, d->W, d->ldx, ho, wo, d->out_scale, d->mean[0],
                                        d->mean[1], d->mean[2], bgr, d->dtype, stream);
            }
            return hat_conv3x3_to_u8(r.P(0), r.P(1), (const float*)r.P(2), dst, dst_pitch, dst_pitch * ho, r.I(4), r.I(5), r.I(6), r.I(7), r.I(8),
                                     ho, wo, r.F(10), (const float*)r.P(11), bgr, r.I(12), stream);
        },
        [&](const float* out, int32_t Hs, int32_t Ws) { return hat_planes_to_u8(out, B, Hs, Ws, dst, dst_pitch, dst_pitch * ho, ho, wo, bgr, stream); });
}

extern "C" int hat_plan_forward_yuv420(const hat_plan* p, const uint8_t* sy, int64_t sy_pitch, int64_t sy_bstride, const uint8_t* scb,
                                       const uint8_t* scr, int64_t sc_pitch, int32_t sc_step, int64_t sc_bstride, int32_t h, int32_t w,
                                       uint8_t* dy, int64_t dy_pitch, int64_t dy_bstride, uint8_t* dcb, uint8_t* dcr, int64_t dc_pitch,
                                       int32_t dc_step, int64_t dc_bstride, const float* to_rgb12, const float* from_rgb12, void* stream) {
    if (!p || !sy || !scb || !scr || !dy || !dcb || !dcr || !to_rgb12 || !from_rgb12 || h < 2 || w < 2 || (h & 1) || (w & 1)) return HAT_EINVAL;
    if ((sc_step != 1 && sc_step != 2) || (dc_step != 1 && dc_step != 2) || sy_pitch < w || sc_pitch < (int64_t)sc_step * (w / 2)) return HAT_EINVAL;
    const HatYuvSurface src = hat_yuv420_surface(sy, sy_pitch, sy_bstride, scb, scr, sc_pitch, sc_step, sc_bstride, 8, 0);
    const HatYuvSurface dst = hat_yuv420_surface(dy, dy_pitch, dy_bstride, dcb, dcr, dc_pitch, dc_step, dc_bstride, 8, 0);
    return forward_yuv(p, &src, &dst, h, w, to_rgb12, from_rgb12, stream, true);
}

// The same forward with a sample width on either side: 8 (bytes, the msb flag is not used) or 10 / 12 / 16 (16-bit words).
extern "C" int hat_plan_forward_yuv420_deep(const hat_plan* p, const void* sy, int64_t sy_pitch, int64_t sy_bstride, const void* scb,
                                            const void* scr, int64_t sc_pitch, int32_t sc_step, int64_t sc_bstride, int32_t src_depth,
                                            int32_t src_msb, int32_t h, int32_t w, void* dy, int64_t dy_pitch, int64_t dy_bstride, void* dcb,
                                            void* dcr, int64_t dc_pitch, int32_t dc_step, int64_t dc_bstride, int32_t dst_depth, int32_t dst_msb,
                                            const float* to_rgb12, const float* from_rgb12, void* stream) {
    if (!p || !sy || !scb || !scr || !dy || !dcb || !dcr || !to_rgb12 || !from_rgb12 || h < 2 || w < 2 || (h & 1) || (w & 1)) return HAT_EINVAL;
    if ((src_depth != 8 && !hat_yuv_depth_ok(src_depth, 0)) || (dst_depth != 8 && !hat_yuv_depth_ok(dst_depth, 0))) return HAT_EINVAL;
    if ((src_msb != 0 && src_msb != 1) || (dst_msb != 0 && dst_msb != 1)) return HAT_EINVAL;
    const int32_t db = dst_depth == 8 ? 1 : 2;
    // before the plan is read: the source block (forward_yuv refuses it, odd pointers included), odd destination pointers and dc_step
    if ((db == 2 && (((uintptr_t)dy | (uintptr_t)dcb | (uintptr_t)dcr) & 1)) || (dc_step != db && dc_step != 2 * db)) return HAT_EINVAL;
    const HatYuvSurface src = hat_yuv420_surface(sy, sy_pitch, sy_bstride, scb, scr, sc_pitch, sc_step, sc_bstride, src_depth, src_msb);
    const HatYuvSurface dst = hat_yuv420_surface(dy, dy_pitch, dy_bstride, dcb, dcr, dc_pitch, dc_step, dc_bstride, dst_depth, dst_msb);
    return forward_yuv(p, &src, &dst, h, w, to_rgb12, from_rgb12, stream, true);
}

// The same forward between two surface descriptions: any subsampling and depth in, any out.
extern "C" int hat_plan_forward_yuv(const hat_plan* p, const HatYuvSurface* src, const HatYuvSurface* dst, int32_t h, int32_t w,
                                    const float* to_rgb12, const float* from_rgb12, void* stream) {
    if (!p || !src || !dst || !to_rgb12 || !from_rgb12 || h < 1 || w < 1) return HAT_EINVAL;
    return forward_yuv(p, src, dst, h, w, to_rgb12, from_rgb12, stream, false);
}

// The same forward with a chroma siting beside each surface; two centre sitings are hat_plan_forward_yuv.
extern "C" int hat_plan_forward_yuv_sited(const hat_plan* p, const HatYuvSurface* src, int32_t src_siting, const HatYuvSurface* dst,
                                          int32_t dst_siting, int32_t h, int32_t w, const float* to_rgb12, const float* from_rgb12,
                                          void* stream) {
    if (!p || !src || !dst || !to_rgb12 || !from_rgb12 || h < 1 || w < 1 || !hat_siting_ok(src_siting) || !hat_siting_ok(dst_siting))
        return HAT_EINVAL;
    return forward_yuv(p, src, dst, h, w, to_rgb12, from_rgb12, stream, false, src_siting, dst_siting);
}

// The same forward with a packed 4:2:2 surface on either side or on both: exactly one of the two pointers of a side is set.
extern "C" int hat_plan_forward_packed422(const hat_plan* p, const HatPackedSurface* src_packed, const HatYuvSurface* src_planar,
                                          int32_t src_siting, const HatPackedSurface* dst_packed, const HatYuvSurface* dst_planar,
                                          int32_t dst_siting, int32_t h, int32_t w, const float* to_rgb12, const float* from_rgb12, void* stream) {
    if (!p || !to_rgb12 || !from_rgb12 || h < 1 || w < 1 || !hat_siting_ok(src_siting) || !hat_siting_ok(dst_siting)) return HAT_EINVAL;
    if (!src_packed == !src_planar || !dst_packed == !dst_planar) return HAT_EINVAL;
    return forward_yuv(p, FrameSide{src_planar, src_packed, src_siting}, FrameSide{dst_planar, dst_packed, dst_siting}, h, w, to_rgb12, from_rgb12,
                       stream, false);
}
