// hat_plan_parse.h — the host half of the plan loader: read a plan file and check ALL of it before anything touches a device.
//
// Plain C++17 over <stdio.h>: no HIP header, no HIP call, nothing but the declarations of include/hat_mi355x.h.  hat_plan.cpp
// includes it (hat_plan_load = hat_plan_parse, then allocate / upload / synchronise); hat_plan_check.cpp builds it with a host
// compiler into a program that says whether a file would load, on machines without a GPU and under host sanitizers.
//
// One list, HAT_PLAN_FUNCTIONS, is the file format's function table: its order gives the function ids (plan.py FN_IDS mirrors
// it), and each entry's C declaration in hat_mi355x.h gives — through the templates below — BOTH the signature table the parser
// checks a recorded call against and the marshalling hat_plan.cpp's dispatch() replays it with.  A call that passes the parser
// therefore holds exactly what the replay reads: the right number of arguments, each of the kind its position takes.
//
// What hat_plan_parse refuses (DESIGN.md "Plan loader rules" lists the same rules; tests/test_plan_parse_cpu.py has one test each):
//   header   wrong magic / short header (EINVAL); version != HAT_ABI_VERSION, n_functions != the table's, n_buffers > 2^20,
//            n_calls > 2^24 (EUNSUPPORTED)
//   dims     B, Cin, H, W, scale, Cout < 1; dtype not HAT_F32 / HAT_BF16; reserved word != 0; scale*H or scale*W past int32;
//            B*3*H*W or B*3*(scale*H)*(scale*W) (the frame entries' staging images, in floats) past INT64_MAX / sizeof(float)
//   buffers  kind > 3; bytes > 2^38; not exactly one input and one output; input bytes != B*Cin*H*W*4; output bytes !=
//            B*Cout*(scale*H)*(scale*W)*4; a constant buffer whose (padded) bytes reach past the end of the file
//   calls    function id outside the table; n_args > 32 or != the function's; an argument whose tag is not its position's kind
//            (so: a stream tag anywhere but last); an int32 position whose value does not fit; a pointer or fixup whose buffer
//            index is out of range or whose offset is past the buffer's bytes (0xFFFFFFFF = NULL is fine); a struct whose size
//            is not sizeof(its descriptor); a host array whose size is not what the entry reads, or that has fixups; more than
//            64 fixups; a fixup whose field offset is not 8-aligned or does not lie wholly inside the struct
//   end      a short read anywhere; bytes after the last call
// All EINVAL unless stated.  The parser allocates host memory in proportion to what it has READ, never to a count it was told.
#ifndef HAT_PLAN_PARSE_H
#define HAT_PLAN_PARSE_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/types.h>

#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/hat_mi355x.h"

namespace hat_plan_host {

enum : uint32_t { ARG_INT = 0, ARG_FLOAT = 1, ARG_PTR = 2, ARG_STRUCT = 3, ARG_HOST = 4, ARG_STREAM = 5 };
enum : uint32_t { BUF_CONST = 0, BUF_SCRATCH = 1, BUF_INPUT = 2, BUF_OUTPUT = 3 };
constexpr uint32_t NULL_BUF = 0xFFFFFFFFu;
constexpr uint64_t MAX_BUF_BYTES = 1ull << 38;   // 256 GiB: above one MI355X's HBM
constexpr uint32_t MAX_ARGS = 32, MAX_FIXUPS = 64, MAX_BLOB_BYTES = 1u << 20;

struct Fix { uint32_t field_off, buf; uint64_t off; };
struct Arg {
    uint32_t tag = 0;
    int64_t i = 0;
    double f = 0;
    uint32_t buf = NULL_BUF;
    uint64_t off = 0;
    std::vector<unsigned char> blob;   // struct image / host array
    std::vector<Fix> fix;
};
struct Call { uint32_t fn; std::vector<Arg> args; };
struct Buf {
    uint32_t kind;
    uint64_t nbytes;
    void* dev = nullptr;     // the loader's: device memory of a constant / scratch buffer
    int64_t file_off = -1;   // constant buffers: where the bytes start in the file (the loader uploads them from there)
};
struct Parsed {
    int32_t dims[8];   // B, Cin, H, W, scale, Cout, dtype, reserved
    std::vector<Buf> bufs;
    std::vector<Call> calls;
};

// ---- the function table --------------------------------------------------------------------------------------------------
// function ids: the order of this list is the file format (super_resolution_amd/plan.py FN_IDS mirrors it)
#define HAT_PLAN_FUNCTIONS(X)                                                                                                        \
    X(hat_conv) X(hat_linear) X(hat_conv3x3_small) X(hat_cab_fold) X(hat_aggr_cab) X(hat_ffn) X(hat_ffn2) X(hat_hab_tail)             \
    X(hat_layernorm) X(hat_esc_weights) X(hat_eca_scale) X(hat_dwconv_gate) X(hat_sgfn_gate) X(hat_ocab_attention)                    \
    X(hat_window_attention) X(hat_cab_squeeze) X(hat_conv3x3_to_planes) X(hat_add_f32) X(hat_esc_conv13) X(hat_ocab_keybias)          \
    X(hat_ocab_attention_kb) X(hat_ocab_mlp) X(hat_ocab_qkv) X(hat_hab_tail3) X(hat_ocab_attention_log2) X(hat_naf_half)              \
    X(hat_naf_fold)

#define HAT_PLAN_ID(f) FN_##f,
enum : uint32_t { HAT_PLAN_FUNCTIONS(HAT_PLAN_ID) N_FN };
#undef HAT_PLAN_ID

// what a position of an entry point takes; K_STREAM is the launch stream, always the last parameter
enum Kind : uint8_t { K_PTR, K_I32, K_I64, K_F32, K_STRUCT, K_HOST, K_STREAM };
struct Param { Kind kind; uint32_t bytes; };   // bytes: sizeof the descriptor (K_STRUCT) / of the host array (K_HOST), else 0
struct Signature { const char* name; uint32_t nargs; Param p[MAX_ARGS]; };

// The one position of the table that C's types cannot tell from a device pointer: hat_conv3x3_to_planes reads its `mean4`
// (four floats) on the HOST while it builds the launch, so a plan carries those bytes instead of a (buffer, offset).
constexpr uint32_t host_array_bytes(uint32_t fn, uint32_t pos) { return fn == FN_hat_conv3x3_to_planes && pos == 11 ? 4 * sizeof(float) : 0; }

template <class T> constexpr Param param_of() {
    if constexpr (std::is_same_v<T, int32_t>) return {K_I32, 0};
    else if constexpr (std::is_same_v<T, int64_t>) return {K_I64, 0};
    else if constexpr (std::is_same_v<T, float>) return {K_F32, 0};
    else {
        static_assert(std::is_pointer_v<T>, "an entry point a plan can record takes int32_t, int64_t, float and pointers only");
        using P = std::remove_cv_t<std::remove_pointer_t<T>>;
        if constexpr (std::is_class_v<P>) return {K_STRUCT, (uint32_t)sizeof(P)};   // a descriptor of hat_mi355x.h, by address
        else return {K_PTR, 0};
    }
}

template <class... A> constexpr Signature signature_of(const char* name, uint32_t fn, int (*)(A...)) {
    static_assert(sizeof...(A) >= 1 && sizeof...(A) <= MAX_ARGS, "argument count");
    Signature s{name, (uint32_t)sizeof...(A), {}};
    const Param ps[] = {param_of<A>()...};
    for (uint32_t k = 0; k < s.nargs; ++k) {
        s.p[k] = ps[k];
        if (const uint32_t hb = host_array_bytes(fn, k)) s.p[k] = {K_HOST, hb};
    }
    s.p[s.nargs - 1].kind = K_STREAM;   // (every launch entry ends with `void* stream`: static_assert below)
    return s;
}

template <class... A> constexpr bool ends_with_stream(int (*)(A...)) {
    using Last = std::tuple_element_t<sizeof...(A) - 1, std::tuple<A...>>;
    return std::is_same_v<Last, void*>;
}

// (a null function pointer of the entry's type: only the TYPE is read, so this header links against nothing)
#define HAT_PLAN_SIG(f) signature_of(#f, FN_##f, (decltype(&f)) nullptr),
inline constexpr Signature SIGNATURES[] = {HAT_PLAN_FUNCTIONS(HAT_PLAN_SIG)};
#undef HAT_PLAN_SIG
#define HAT_PLAN_ASSERT(f) static_assert(ends_with_stream((decltype(&f)) nullptr), #f ": the last parameter must be void* stream");
HAT_PLAN_FUNCTIONS(HAT_PLAN_ASSERT)
#undef HAT_PLAN_ASSERT
static_assert(sizeof(SIGNATURES) / sizeof(SIGNATURES[0]) == N_FN, "one signature per function id");
static_assert(sizeof(void*) == 8, "fixups patch 8-byte pointer fields");

inline const char* kind_name(Kind k) {
    switch (k) {
        case K_PTR: return "ptr";
        case K_I32: return "i32";
        case K_I64: return "i64";
        case K_F32: return "f32";
        case K_STRUCT: return "struct";
        case K_HOST: return "host";
        default: return "stream";
    }
}

// ---- the parser ----------------------------------------------------------------------------------------------------------
struct Reader {
    FILE* f;
    bool ok = true;
    template <typename T> T get() { T v{}; if (fread(&v, sizeof(T), 1, f) != 1) ok = false; return v; }
    void bytes(void* p, size_t n) { if (n && fread(p, 1, n, f) != n) ok = false; }
};

// (buffer, offset) must point INTO the buffer (one-past-the-end is allowed for empty views)
inline bool ptr_ok(const std::vector<Buf>& bufs, uint32_t buf, uint64_t off) {
    if (buf == NULL_BUF) return true;
    return buf < bufs.size() && off <= bufs[buf].nbytes;
}

// a * b for non-negative operands, false when it does not fit an int64_t
inline bool mul_ok(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }

// dims -> the byte sizes hat_plan_forward's caller owes: x = B*Cin*H*W floats, y = B*Cout*(s H)*(s W) floats
inline int check_dims(const int32_t* d, uint64_t* in_bytes, uint64_t* out_bytes) {
    for (int k = 0; k < 6; ++k)
        if (d[k] < 1) return HAT_EINVAL;
    if ((d[6] != HAT_F32 && d[6] != HAT_BF16) || d[7] != 0) return HAT_EINVAL;
    const int64_t B = d[0], Cin = d[1], H = d[2], W = d[3], s = d[4], Cout = d[5], sH = s * H, sW = s * W;   // (int32 x int32: no overflow)
    if (sH > INT32_MAX || sW > INT32_MAX) return HAT_EINVAL;   // the frame entries pass scale*h, scale*w as int32_t
    const int64_t cap = INT64_MAX / (int64_t)sizeof(float);
    int64_t lr = 0, hr = 0, v = 0;
    if (!mul_ok(H, W, &lr) || !mul_ok(lr, B, &lr) || !mul_ok(sH, sW, &hr) || !mul_ok(hr, B, &hr)) return HAT_EINVAL;
    // the two staging images of the frame entries (three planes each) ...
    if (!mul_ok(lr, 3, &v) || v > cap || !mul_ok(hr, 3, &v) || v > cap) return HAT_EINVAL;
    // ... and the caller's x and y
    if (!mul_ok(lr, Cin, &v) || v > cap) return HAT_EINVAL;
    *in_bytes = (uint64_t)v * sizeof(float);
    if (!mul_ok(hr, Cout, &v) || v > cap) return HAT_EINVAL;
    *out_bytes = (uint64_t)v * sizeof(float);
    return 0;
}

// Reads the whole plan from f (opened "rb", at its start) into *out and checks every rule at the top of this file.
// Returns 0, HAT_EINVAL or HAT_EUNSUPPORTED.  May throw std::bad_alloc (the callers sit behind a catch).
inline int hat_plan_parse(FILE* f, Parsed* out) {
    if (fseeko(f, 0, SEEK_END) != 0) return HAT_EINVAL;
    const off_t file_len = ftello(f);
    if (file_len < 0 || fseeko(f, 0, SEEK_SET) != 0) return HAT_EINVAL;
    Reader rd{f};
    char magic[8];
    rd.bytes(magic, 8);
    if (!rd.ok || memcmp(magic, "HATPLAN1", 8) != 0) return HAT_EINVAL;
    const uint32_t version = rd.get<uint32_t>(), nbuf = rd.get<uint32_t>(), ncall = rd.get<uint32_t>(), nfn = rd.get<uint32_t>();
    if (!rd.ok) return HAT_EINVAL;
    // version = HAT_ABI_VERSION of the writer: the calls embed raw images of this header's descriptors
    if (version != HAT_ABI_VERSION || nfn != N_FN || nbuf > (1u << 20) || ncall > (1u << 24)) return HAT_EUNSUPPORTED;
    for (int i = 0; i < 8; ++i) out->dims[i] = rd.get<int32_t>();
    if (!rd.ok) return HAT_EINVAL;
    uint64_t in_bytes = 0, out_bytes = 0;
    if (const int rc = check_dims(out->dims, &in_bytes, &out_bytes)) return rc;

    uint32_t n_in = 0, n_out = 0;
    for (uint32_t i = 0; i < nbuf; ++i) {
        Buf b;
        b.kind = rd.get<uint32_t>();
        (void)rd.get<uint32_t>();
        b.nbytes = rd.get<uint64_t>();
        if (!rd.ok || b.kind > BUF_OUTPUT || b.nbytes > MAX_BUF_BYTES) return HAT_EINVAL;
        if (b.kind == BUF_INPUT && (++n_in > 1 || b.nbytes != in_bytes)) return HAT_EINVAL;
        if (b.kind == BUF_OUTPUT && (++n_out > 1 || b.nbytes != out_bytes)) return HAT_EINVAL;
        if (b.kind == BUF_CONST) {   // the bytes stay in the file: the loader uploads them once everything has passed
            const off_t at = ftello(f);
            const uint64_t padded = (b.nbytes + 7) / 8 * 8;   // (nbytes <= 2^38: no overflow)
            if (at < 0 || padded > (uint64_t)(file_len - at)) return HAT_EINVAL;
            b.file_off = (int64_t)at;
            if (fseeko(f, (off_t)padded, SEEK_CUR) != 0) return HAT_EINVAL;
        }
        out->bufs.push_back(b);
    }
    if (n_in != 1 || n_out != 1) return HAT_EINVAL;

    for (uint32_t i = 0; i < ncall; ++i) {
        Call c;
        c.fn = rd.get<uint32_t>();
        const uint32_t nargs = rd.get<uint32_t>();
        if (!rd.ok || c.fn >= N_FN || nargs > MAX_ARGS) return HAT_EINVAL;
        const Signature& sig = SIGNATURES[c.fn];
        if (nargs != sig.nargs) return HAT_EINVAL;
        for (uint32_t k = 0; k < nargs; ++k) {
            const Param want = sig.p[k];
            Arg a;
            a.tag = rd.get<uint32_t>();
            (void)rd.get<uint32_t>();
            if (!rd.ok) return HAT_EINVAL;
            switch (want.kind) {
                case K_I32:
                case K_I64:
                    if (a.tag != ARG_INT) return HAT_EINVAL;
                    a.i = rd.get<int64_t>();
                    if (want.kind == K_I32 && (a.i < INT32_MIN || a.i > INT32_MAX)) return HAT_EINVAL;
                    break;
                case K_F32:
                    if (a.tag != ARG_FLOAT) return HAT_EINVAL;
                    a.f = rd.get<double>();
                    break;
                case K_PTR:
                    if (a.tag != ARG_PTR) return HAT_EINVAL;
                    a.buf = rd.get<uint32_t>();
                    (void)rd.get<uint32_t>();
                    a.off = rd.get<uint64_t>();
                    if (!rd.ok || !ptr_ok(out->bufs, a.buf, a.off)) return HAT_EINVAL;
                    break;
                case K_STRUCT:
                case K_HOST: {
                    if (a.tag != (want.kind == K_STRUCT ? ARG_STRUCT : ARG_HOST)) return HAT_EINVAL;
                    const uint32_t nb = rd.get<uint32_t>(), nfix = rd.get<uint32_t>();
                    if (!rd.ok || nb > MAX_BLOB_BYTES || nfix > MAX_FIXUPS) return HAT_EINVAL;
                    if (nb != want.bytes || (want.kind == K_HOST && nfix != 0)) return HAT_EINVAL;
                    a.blob.resize((nb + 7) / 8 * 8);
                    rd.bytes(a.blob.data(), a.blob.size());
                    for (uint32_t j = 0; j < nfix; ++j) {
                        Fix fx;
                        fx.field_off = rd.get<uint32_t>();
                        fx.buf = rd.get<uint32_t>();
                        fx.off = rd.get<uint64_t>();
                        if (!rd.ok || fx.field_off % 8 != 0 || (uint64_t)fx.field_off + sizeof(void*) > nb || !ptr_ok(out->bufs, fx.buf, fx.off))
                            return HAT_EINVAL;
                        a.fix.push_back(fx);
                    }
                    break;
                }
                default:   // K_STREAM: no payload
                    if (a.tag != ARG_STREAM) return HAT_EINVAL;
                    break;
            }
            if (!rd.ok) return HAT_EINVAL;
            c.args.push_back(std::move(a));
        }
        out->calls.push_back(std::move(c));
    }
    if (!rd.ok || ftello(f) != file_len) return HAT_EINVAL;   // (bytes after the last call: not a file the exporter wrote)
    return 0;
}

}  // namespace hat_plan_host

#endif
