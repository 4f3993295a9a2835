/* examples/plan_upscale_u8.c — upscale an 8-bit image from C: read a binary PPM, run a forward plan on it, write a PPM.
 *
 *   python -m super_resolution_amd.plan -opt options/test/HAT-S_SRx4.yml --shape 1 720 1280 -o hats_720p.hatplan   (once)
 *   gcc examples/plan_upscale_u8.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lsuper_resolution_amd -lhat_mi355x \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/super_resolution_amd -o plan_upscale_u8
 *   ./plan_upscale_u8 hats_720p.hatplan in.ppm out.ppm
 *
 * The image may be smaller than the plan's shape (down to just over half of it on each side): hat_plan_forward_u8
 * reflect-pads it on the device, and crops the result.  The plan must be recorded for batch 1.  Only the C ABI of
 * include/hat_mi355x.h and the HIP runtime are used: no image library.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hat_mi355x.h"

/* the next unsigned integer of a PPM header, skipping white space and '#' comments; -1 on error */
static long ppm_int(FILE* f) {
    int c = fgetc(f);
    while (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '#') {
        if (c == '#')
            while (c != '\n' && c != EOF) c = fgetc(f);
        c = fgetc(f);
    }
    if (c < '0' || c > '9') return -1;
    long v = 0;
    while (c >= '0' && c <= '9' && v < 100000000L) { v = v * 10 + (c - '0'); c = fgetc(f); }
    return v;   /* the one white-space byte after the number has been consumed (what the format asks after maxval) */
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s net.hatplan in.ppm out.ppm\n", argv[0]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    if (fgetc(f) != 'P' || fgetc(f) != '6') { fprintf(stderr, "%s is not a binary PPM (P6)\n", argv[2]); return 1; }
    const long w = ppm_int(f), h = ppm_int(f), maxval = ppm_int(f);
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || maxval != 255) { fprintf(stderr, "need an 8-bit P6 image (maxval 255)\n"); return 1; }
    const size_t nin = (size_t)h * w * 3;
    uint8_t* hin = (uint8_t*)malloc(nin);
    if (!hin || fread(hin, 1, nin, f) != nin) { fprintf(stderr, "%s is truncated\n", argv[2]); return 1; }
    fclose(f);

    hat_plan* plan = NULL;
    int rc = hat_plan_load(argv[1], &plan);
    if (rc) { fprintf(stderr, "hat_plan_load failed: %d\n", rc); return 1; }
    int32_t d[8];
    hat_plan_info(plan, d, NULL, NULL);
    if (d[0] != 1) { fprintf(stderr, "the plan is recorded for batch %d: this example upscales one image\n", d[0]); return 1; }
    const int s = d[4];
    const size_t nout = nin * s * s;
    uint8_t *hout = (uint8_t*)malloc(nout), *din = NULL, *dout = NULL;
    if (!hout || hipMalloc((void**)&din, nin) || hipMalloc((void**)&dout, nout) || hipMemcpy(din, hin, nin, hipMemcpyHostToDevice)) return 1;
    /* rows are packed on both sides: pitch = 3 bytes x width; flags 0 = R, G, B byte order (PPM's) */
    rc = hat_plan_forward_u8(plan, din, 3 * w, (int32_t)h, (int32_t)w, dout, 3 * w * s, 0, NULL);
    if (rc) { fprintf(stderr, "hat_plan_forward_u8 failed: %d (plan shape %dx%d, image %ldx%ld)\n", rc, d[2], d[3], h, w); return 1; }
    if (hipDeviceSynchronize() || hipMemcpy(hout, dout, nout, hipMemcpyDeviceToHost)) return 1;
    f = fopen(argv[3], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    fprintf(f, "P6\n%ld %ld\n255\n", w * s, h * s);
    if (fwrite(hout, 1, nout, f) != nout || fclose(f)) { fprintf(stderr, "write to %s failed\n", argv[3]); return 1; }
    printf("%ldx%ld -> %ldx%ld\n", w, h, w * s, h * s);
    hat_plan_free(plan);
    (void)hipFree(din);
    (void)hipFree(dout);
    free(hin);
    free(hout);
    return 0;
}
