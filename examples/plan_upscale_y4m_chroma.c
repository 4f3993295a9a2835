/* examples/plan_upscale_y4m_chroma.c — plan_upscale_y4m.c for every chroma subsampling: read a YUV4MPEG2 file of 4:2:0, 4:2:2,
 * 4:4:4 or grey video, run a forward plan on every frame, write the subsampling asked for.
 *
 *   python -m super_resolution_amd.plan -opt options/test/HAT-S_SRx4.yml --shape 1 720 1280 -o hats_720p.hatplan   (once)
 *   gcc examples/plan_upscale_y4m_chroma.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lsuper_resolution_amd -lhat_mi355x \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/super_resolution_amd -o plan_upscale_y4m_chroma
 *   ./plan_upscale_y4m_chroma hats_720p.hatplan in.y4m out.y4m [420|422|444|mono [out_depth]] [--chroma-loc center|left|topleft]
 *
 * Input: C420 (jpeg, mpeg2, paldv, or no C token), C422, C444, Cmono and their deep forms C420p10 / C422p12 / C444p16 / Cmono10 ...
 * (little-endian 16-bit words, the code LSB-aligned).  The third argument is the output's subsampling (default: the input's), the
 * fourth its sample width (default: the input's): `444` on a 4:2:0 file keeps all of the network's chroma.  One HatYuvSurface
 * describes each side and hat_plan_forward_yuv converts on the device with the BT.601 limited-range matrices below.  The frames
 * --chroma-loc names the chroma siting of both sides (include/hat_mi355x.h, "Chroma siting"): center, the default, is this example as
 * it always was; left (MPEG-2, H.264, HEVC, AV1; all standard 4:2:2) and topleft (BT.2020) go through hat_plan_forward_yuv_sited,
 * and an 8-bit 4:2:0 output then says C420mpeg2 / C420paldv.  The frames
 * may be smaller than the plan's shape (down to just over half of it on each side).  The plan must be recorded for batch 1.  Only
 * the C ABI of include/hat_mi355x.h and the HIP runtime are used.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hat_mi355x.h"

/* super_resolution_amd.yuv.csc('bt601', False): rows R, G, B x columns Y, Cb - 128, Cr - 128, offset; rows Y, Cb, Cr x R, G, B, offset */
static const float TO_RGB[12] = {0.00456621f, 0.0f, 0.00625893f, -0.07305696f, 0.00456621f, -0.00153632f, -0.00318811f, -0.07305645f,
                                 0.00456621f, 0.00791071f, 0.0f, -0.07306049f};
static const float FROM_RGB[12] = {65.481f, 128.553f, 24.966f, 16.0f, -37.797f, -74.203f, 112.0f, 128.0f, 112.0f, -93.786f, -18.214f, 128.0f};

enum { C420, C422, C444, CMONO };
static const char* const NAMES[4] = {"420", "422", "444", "mono"};

/* the C token (without its C) -> subsampling and depth; 0 if it is none of this example's */
static int parse_c(const char* t, int* sub, int* depth) {
    static const char* const sited[3] = {"420jpeg", "420mpeg2", "420paldv"};
    for (int i = 0; i < 3; ++i)
        if (!strcmp(t, sited[i])) { *sub = C420, *depth = 8; return 1; }
    for (int s = 0; s < 4; ++s) {
        const size_t n = strlen(NAMES[s]);
        if (strncmp(t, NAMES[s], n)) continue;
        const char* r = t + n;
        if (!*r) { *sub = s, *depth = 8; return 1; }
        if (s != CMONO) { if (*r != 'p') return 0; ++r; }
        if (!strcmp(r, "10") || !strcmp(r, "12") || !strcmp(r, "16")) { *sub = s, *depth = atoi(r); return 1; }
        return 0;
    }
    return 0;
}

/* samples of one h x w frame, and its surface over the packed planes at base (planar chroma: Cb follows Y, Cr follows Cb; pitches
   and steps in BYTES; batch strides unused, B = 1; the words of a Y4M file are LSB-aligned, msb = 0) */
static size_t frame_samples(int sub, long h, long w) {
    const long cw = sub == C444 ? w : w / 2, ch = sub == C420 ? h / 2 : h;
    return (size_t)w * h + (sub == CMONO ? 0 : 2 * (size_t)cw * ch);
}

static HatYuvSurface surface(uint8_t* base, int sub, int depth, long h, long w) {
    const long b = depth == 8 ? 1 : 2, cw = sub == C444 ? w : w / 2, ch = sub == C420 ? h / 2 : h;
    HatYuvSurface s;
    memset(&s, 0, sizeof s);
    s.y = base, s.y_pitch = w * b, s.depth = depth, s.msb = 0;
    if (sub != CMONO) {
        s.cb = base + w * h * b, s.cr = base + (w * h + cw * ch) * b;
        s.c_pitch = cw * b, s.c_step = (int32_t)b, s.sub_x = sub != C444, s.sub_y = sub == C420;
    }
    return s;
}

int main(int argc, char** argv) {
    static const char* const LOCS[3] = {"center", "left", "topleft"};
    static const char* const LOC_TOKENS[3] = {"C420jpeg", "C420mpeg2", "C420paldv"};
    int siting = HAT_SITING_CENTER;
    for (int i = 1; i < argc; ++i) {   /* --chroma-loc <name> may stand anywhere; it is taken out of the positional arguments */
        if (strcmp(argv[i], "--chroma-loc")) continue;
        for (siting = 0; i + 1 < argc && siting < 3 && strcmp(argv[i + 1], LOCS[siting]); ++siting) {}
        if (i + 1 >= argc || siting == 3) { fprintf(stderr, "--chroma-loc is center, left or topleft\n"); return 2; }
        for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
        argc -= 2, --i;
    }
    if (argc < 4) {
        fprintf(stderr, "usage: %s net.hatplan in.y4m out.y4m [420|422|444|mono [out_depth]] [--chroma-loc center|left|topleft]\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    char head[4096], rest[4096] = "", in_c[32] = "";
    if (!fgets(head, sizeof head, f) || strncmp(head, "YUV4MPEG2", 9) != 0 || !strchr(head, '\n')) { fprintf(stderr, "%s is not a YUV4MPEG2 file\n", argv[2]); return 1; }
    long w = 0, h = 0;
    int sub = C420, depth = 8;
    for (char* tok = strtok(head + 9, " \n"); tok; tok = strtok(NULL, " \n")) {
        if (tok[0] == 'W') w = atol(tok + 1);
        else if (tok[0] == 'H') h = atol(tok + 1);
        else if (tok[0] == 'C') {
            if (!parse_c(tok + 1, &sub, &depth) || strlen(tok) >= sizeof in_c) { fprintf(stderr, "colour space %s is not supported\n", tok); return 1; }
            strcpy(in_c, tok);
        } else {   /* every other token is copied to the output header */
            const size_t used = strlen(rest), need = strlen(tok) + 2;
            if (used + need > sizeof rest) { fprintf(stderr, "the header of %s is too long\n", argv[2]); return 1; }
            rest[used] = ' ';
            memcpy(rest + used + 1, tok, need - 1);
        }
    }
    int out_sub = sub, out_depth = depth;
    if (argc > 4) {
        for (out_sub = 0; out_sub < 4 && strcmp(argv[4], NAMES[out_sub]); ++out_sub) {}
        if (out_sub == 4) { fprintf(stderr, "the output subsampling is 420, 422, 444 or mono, got %s\n", argv[4]); return 1; }
    }
    if (argc > 5) out_depth = atoi(argv[5]);
    if (out_depth != 8 && out_depth != 10 && out_depth != 12 && out_depth != 16) { fprintf(stderr, "out_depth is 8, 10, 12 or 16, got %s\n", argv[5]); return 1; }
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || (sub != C444 && sub != CMONO && w % 2) || (sub == C420 && h % 2)) {
        fprintf(stderr, "a C%s frame cannot be %ldx%ld\n", NAMES[sub], w, h);
        return 1;
    }
    char out_c[32] = "";   /* an unchanged subsampling and depth keep the input's token (C420jpeg stays C420jpeg, none stays none) */
    if (out_sub == sub && out_depth == depth) strcpy(out_c, in_c);
    else if (out_depth == 8) sprintf(out_c, "C%s", NAMES[out_sub]);
    else sprintf(out_c, out_sub == CMONO ? "C%s%d" : "C%sp%d", NAMES[out_sub], out_depth % 100);
    if (siting != HAT_SITING_CENTER && out_sub == C420 && out_depth == 8) strcpy(out_c, LOC_TOKENS[siting]);   /* the header says what is written */

    hat_plan* plan = NULL;
    int rc = hat_plan_load(argv[1], &plan);
    if (rc) { fprintf(stderr, "hat_plan_load failed: %d\n", rc); return 1; }
    int32_t d[8];
    hat_plan_info(plan, d, NULL, NULL);
    if (d[0] != 1) { fprintf(stderr, "the plan is recorded for batch %d: this example upscales one frame at a time\n", d[0]); return 1; }
    const long s = d[4], W = w * s, H = h * s;
    if (((out_sub == C420 || out_sub == C422) && W % 2) || (out_sub == C420 && H % 2)) { fprintf(stderr, "a C%s frame cannot be %ldx%ld\n", NAMES[out_sub], W, H); return 1; }
    const size_t nin = frame_samples(sub, h, w) * (depth == 8 ? 1 : 2), nout = frame_samples(out_sub, H, W) * (out_depth == 8 ? 1 : 2);
    uint8_t *hin = (uint8_t*)malloc(nin), *hout = (uint8_t*)malloc(nout), *din = NULL, *dout = NULL;
    if (!hin || !hout || hipMalloc((void**)&din, nin) || hipMalloc((void**)&dout, nout)) return 1;
    const HatYuvSurface src = surface(din, sub, depth, h, w), dst = surface(dout, out_sub, out_depth, H, W);
    FILE* g = fopen(argv[3], "wb");
    if (!g) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    /* the C token goes where ffmpeg and mjpegtools write it: after the tokens copied from the input */
    fprintf(g, "YUV4MPEG2 W%ld H%ld%s%s%s\n", W, H, rest, out_c[0] ? " " : "", out_c);

    char line[256];
    long frames = 0;
    while (fgets(line, sizeof line, f)) {
        if (strncmp(line, "FRAME", 5) != 0 || !strchr(line, '\n')) { fprintf(stderr, "frame %ld: expected a FRAME record\n", frames); return 1; }
        if (fread(hin, 1, nin, f) != nin) { fprintf(stderr, "frame %ld is truncated\n", frames); return 1; }
        if (hipMemcpy(din, hin, nin, hipMemcpyHostToDevice)) return 1;
        rc = siting == HAT_SITING_CENTER ? hat_plan_forward_yuv(plan, &src, &dst, (int32_t)h, (int32_t)w, TO_RGB, FROM_RGB, NULL)
                                         : hat_plan_forward_yuv_sited(plan, &src, siting, &dst, siting, (int32_t)h, (int32_t)w, TO_RGB, FROM_RGB, NULL);
        if (rc) { fprintf(stderr, "hat_plan_forward_yuv failed: %d (plan shape %dx%d, frame %ldx%ld)\n", rc, d[2], d[3], h, w); return 1; }
        if (hipDeviceSynchronize() || hipMemcpy(hout, dout, nout, hipMemcpyDeviceToHost)) return 1;
        if (fputs("FRAME\n", g) < 0 || fwrite(hout, 1, nout, g) != nout) { fprintf(stderr, "write to %s failed\n", argv[3]); return 1; }
        ++frames;
    }
    if (fclose(g)) { fprintf(stderr, "write to %s failed\n", argv[3]); return 1; }
    fclose(f);
    printf("%ld frames C%s %ldx%ld -> C%s %ldx%ld\n", frames, NAMES[sub], w, h, NAMES[out_sub], W, H);
    hat_plan_free(plan);
    (void)hipFree(din);
    (void)hipFree(dout);
    free(hin);
    free(hout);
    return 0;
}
