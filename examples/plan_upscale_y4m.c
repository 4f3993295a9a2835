/* examples/plan_upscale_y4m.c — upscale a video from C: read a YUV4MPEG2 file, run a forward plan on every frame, write one.
 *
 *   python -m super_resolution_amd.plan -opt options/test/HAT-S_SRx4.yml --shape 1 720 1280 -o hats_720p.hatplan   (once)
 *   gcc examples/plan_upscale_y4m.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lsuper_resolution_amd -lhat_mi355x \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/super_resolution_amd -o plan_upscale_y4m
 *   ./plan_upscale_y4m hats_720p.hatplan in.y4m out.y4m [out_depth]
 *
 * 4:2:0 only: 8-bit (C420, C420jpeg, C420mpeg2, C420paldv, or no C token) or C420p10 / C420p12 / C420p16 (little-endian 16-bit
 * words, the code LSB-aligned).  out_depth (8, 10, 12 or 16; default: the input's) is the sample width of the output file: 10
 * on an 8-bit input writes the network's result with ten bits.  The frames go up and come back as they lie in
 * the file — Y, Cb, Cr planes — and hat_plan_forward_yuv420_deep converts on the device with the BT.601 limited-range matrices
 * below, which are the same at every depth (super_resolution_amd.yuv.csc() prints others).  The frames may be smaller than the plan's shape (down to just
 * over half of it on each side).  The plan must be recorded for batch 1.  Only the C ABI of include/hat_mi355x.h and the
 * HIP runtime are used.
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

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s net.hatplan in.y4m out.y4m [out_depth]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    char head[4096], rest[4096] = "";
    if (!fgets(head, sizeof head, f) || strncmp(head, "YUV4MPEG2", 9) != 0 || !strchr(head, '\n')) { fprintf(stderr, "%s is not a YUV4MPEG2 file\n", argv[2]); return 1; }
    long w = 0, h = 0;
    int depth = 8, have_c = 0;
    const int want = argc > 4 ? atoi(argv[4]) : 0;   /* 0: the input's depth */
    char ctok[16];
    for (char* tok = strtok(head + 9, " \n"); tok; tok = strtok(NULL, " \n")) {
        if (tok[0] == 'W') w = atol(tok + 1);
        else if (tok[0] == 'H') h = atol(tok + 1);
        else {
            if (tok[0] == 'C') {
                if (!strcmp(tok, "C420p10")) depth = 10;
                else if (!strcmp(tok, "C420p12")) depth = 12;
                else if (!strcmp(tok, "C420p16")) depth = 16;
                else if (strcmp(tok, "C420") && strcmp(tok, "C420jpeg") && strcmp(tok, "C420mpeg2") && strcmp(tok, "C420paldv")) {
                    fprintf(stderr, "colour space %s is not supported: 4:2:0 with 8, 10, 12 or 16 bits only\n", tok);
                    return 1;
                }
                if (want && want != depth) {   /* the output's C token names the output's depth; an unchanged depth keeps the token */
                    sprintf(ctok, want == 8 ? "C420" : "C420p%d", want % 100);
                    tok = ctok;
                }
                have_c = 1;
            }
            const size_t used = strlen(rest), need = strlen(tok) + 2;   /* every other token is copied to the output header */
            if (used + need > sizeof rest) { fprintf(stderr, "the header of %s is too long\n", argv[2]); return 1; }
            rest[used] = ' ';
            memcpy(rest + used + 1, tok, need - 1);
        }
    }
    const int out_depth = want ? want : depth;
    if (out_depth != 8 && out_depth != 10 && out_depth != 12 && out_depth != 16) { fprintf(stderr, "out_depth is 8, 10, 12 or 16, got %s\n", argv[4]); return 1; }
    if (!have_c && out_depth != 8) {   /* no C token means 8 bits */
        const size_t used = strlen(rest);
        if (used + 10 > sizeof rest) { fprintf(stderr, "the header of %s is too long\n", argv[2]); return 1; }
        sprintf(rest + used, " C420p%d", out_depth);
    }
    if (w < 2 || h < 2 || w > 65534 || h > 65534 || w % 2 || h % 2) { fprintf(stderr, "need even W and H, got %ldx%ld\n", w, h); return 1; }

    hat_plan* plan = NULL;
    int rc = hat_plan_load(argv[1], &plan);
    if (rc) { fprintf(stderr, "hat_plan_load failed: %d\n", rc); return 1; }
    int32_t d[8];
    hat_plan_info(plan, d, NULL, NULL);
    if (d[0] != 1) { fprintf(stderr, "the plan is recorded for batch %d: this example upscales one frame at a time\n", d[0]); return 1; }
    const long s = d[4], W = w * s, H = h * s;
    const long bi = depth == 8 ? 1 : 2, bo = out_depth == 8 ? 1 : 2;   /* bytes per sample */
    const size_t nin = (size_t)w * h * 3 / 2 * bi, nout = (size_t)W * H * 3 / 2 * bo;
    uint8_t *hin = (uint8_t*)malloc(nin), *hout = (uint8_t*)malloc(nout), *din = NULL, *dout = NULL;
    if (!hin || !hout || hipMalloc((void**)&din, nin) || hipMalloc((void**)&dout, nout)) return 1;
    FILE* g = fopen(argv[3], "wb");
    if (!g) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    fprintf(g, "YUV4MPEG2 W%ld H%ld%s\n", W, H, rest);

    char line[256];
    long frames = 0;
    while (fgets(line, sizeof line, f)) {
        if (strncmp(line, "FRAME", 5) != 0 || !strchr(line, '\n')) { fprintf(stderr, "frame %ld: expected a FRAME record\n", frames); return 1; }
        if (fread(hin, 1, nin, f) != nin) { fprintf(stderr, "frame %ld is truncated\n", frames); return 1; }
        if (hipMemcpy(din, hin, nin, hipMemcpyHostToDevice)) return 1;
        /* planar chroma on both sides: Cb follows Y, Cr follows Cb; rows are packed; chroma step one sample; pitches and steps in
           BYTES; batch strides unused (B = 1); the words of a Y4M file are LSB-aligned (msb = 0) */
        rc = hat_plan_forward_yuv420_deep(plan, din, w * bi, 0, din + w * h * bi, din + (w * h + (w / 2) * (h / 2)) * bi, w / 2 * bi, (int32_t)bi, 0,
                                          depth, 0, (int32_t)h, (int32_t)w, dout, W * bo, 0, dout + W * H * bo,
                                          dout + (W * H + (W / 2) * (H / 2)) * bo, W / 2 * bo, (int32_t)bo, 0, out_depth, 0, TO_RGB, FROM_RGB, NULL);
        if (rc) { fprintf(stderr, "hat_plan_forward_yuv420_deep failed: %d (plan shape %dx%d, frame %ldx%ld)\n", rc, d[2], d[3], h, w); return 1; }
        if (hipDeviceSynchronize() || hipMemcpy(hout, dout, nout, hipMemcpyDeviceToHost)) return 1;
        if (fputs("FRAME\n", g) < 0 || fwrite(hout, 1, nout, g) != nout) { fprintf(stderr, "write to %s failed\n", argv[3]); return 1; }
        ++frames;
    }
    if (fclose(g)) { fprintf(stderr, "write to %s failed\n", argv[3]); return 1; }
    fclose(f);
    printf("%ld frames %ldx%ld -> %ldx%ld\n", frames, w, h, W, H);
    hat_plan_free(plan);
    (void)hipFree(din);
    (void)hipFree(dout);
    free(hin);
    free(hout);
    return 0;
}
