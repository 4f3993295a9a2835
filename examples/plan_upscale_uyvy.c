/* examples/plan_upscale_uyvy.c — upscale packed 4:2:2 video from C: read a headerless UYVY file, run a forward plan on every
 * frame, write a headerless UYVY file (`ffmpeg -f rawvideo -pix_fmt uyvy422 -s WxH`).
 *
 *   python -m super_resolution_amd.plan -opt options/test/HAT-S_SRx4.yml --shape 1 720 1280 -o hats_720p.hatplan   (once)
 *   gcc examples/plan_upscale_uyvy.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Lsuper_resolution_amd -lhat_mi355x \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/super_resolution_amd -o plan_upscale_uyvy
 *   ./plan_upscale_uyvy hats_720p.hatplan --size 720 1280 in.uyvy out.uyvy [--left]
 *
 * --size H W: the size of the file's frames (W even), which the file does not say; it may be smaller than the plan's shape (down
 * to just over half of it on each side).  The colour matrix is BT.601 limited range, the twelve floats yuv.csc("bt601") prints;
 * --left: left-sited chroma on both sides (standard 4:2:2), default centre.  The plan must be recorded for batch 1.  Only the C ABI
 * of include/hat_mi355x.h and the HIP runtime are used.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hat_mi355x.h"

/* yuv.csc("bt601", full_range=False): rows R, G, B over Y, Cb - 128, Cr - 128, offset; rows Y, Cb, Cr over R, G, B, offset */
static const float TO_RGB[12] = {0.00456621f, 0.0f, 0.00625893f, -0.07305696f, 0.00456621f, -0.00153632f, -0.00318811f, -0.07305645f,
                                 0.00456621f, 0.00791071f, 0.0f, -0.07306049f};
static const float FROM_RGB[12] = {65.481f, 128.553f, 24.966f, 16.0f, -37.797f, -74.203f, 112.0f, 128.0f, 112.0f, -93.786f, -18.214f, 128.0f};

int main(int argc, char** argv) {
    long h = 0, w = 0;
    int siting = HAT_SITING_CENTER, npos = 0;
    const char* pos[3] = {NULL, NULL, NULL};
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--size") && i + 2 < argc) { h = atol(argv[i + 1]); w = atol(argv[i + 2]); i += 2; }
        else if (!strcmp(argv[i], "--left")) siting = HAT_SITING_LEFT;
        else if (npos < 3) pos[npos++] = argv[i];
        else npos = 4;
    }
    if (npos != 3 || h < 1 || w < 2 || (w & 1) || h > 65535 || w > 65535) {
        fprintf(stderr, "usage: %s net.hatplan --size H W in.uyvy out.uyvy [--left]   (W even)\n", argv[0]);
        return 2;
    }
    hat_plan* plan = NULL;
    int rc = hat_plan_load(pos[0], &plan);
    if (rc) { fprintf(stderr, "hat_plan_load failed: %d\n", rc); return 1; }
    int32_t d[8];
    hat_plan_info(plan, d, NULL, NULL);
    if (d[0] != 1) { fprintf(stderr, "the plan is recorded for batch %d: this example upscales one frame at a time\n", d[0]); return 1; }
    const int s = d[4];
    const size_t nin = (size_t)h * w * 2, nout = nin * s * s;   /* two bytes a pixel on both sides */
    FILE* fi = fopen(pos[1], "rb");
    FILE* fo = fopen(pos[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open %s\n", fi ? pos[2] : pos[1]); return 1; }
    uint8_t *hin = (uint8_t*)malloc(nin), *hout = (uint8_t*)malloc(nout), *din = NULL, *dout = NULL;
    if (!hin || !hout || hipMalloc((void**)&din, nin) || hipMalloc((void**)&dout, nout)) return 1;
    /* rows are packed on both sides: pitch = 2 bytes x width; one frame a call, so the batch stride is not read */
    const HatPackedSurface src = {din, 2 * w, 0, HAT_PACKED_UYVY, 8, 0, 0};
    const HatPackedSurface dst = {dout, 2 * w * s, 0, HAT_PACKED_UYVY, 8, 0, 0};
    long frames = 0;
    size_t got;
    while ((got = fread(hin, 1, nin, fi)) == nin) {
        if (hipMemcpy(din, hin, nin, hipMemcpyHostToDevice)) return 1;
        rc = hat_plan_forward_packed422(plan, &src, NULL, siting, &dst, NULL, siting, (int32_t)h, (int32_t)w, TO_RGB, FROM_RGB, NULL);
        if (rc) { fprintf(stderr, "hat_plan_forward_packed422 failed: %d (plan shape %dx%d, frame %ldx%ld)\n", rc, d[2], d[3], h, w); return 1; }
        if (hipDeviceSynchronize() || hipMemcpy(hout, dout, nout, hipMemcpyDeviceToHost)) return 1;
        if (fwrite(hout, 1, nout, fo) != nout) { fprintf(stderr, "write to %s failed\n", pos[2]); return 1; }
        ++frames;
    }
    if (got) { fprintf(stderr, "%s ends inside a frame (%zu of %zu bytes)\n", pos[1], got, nin); return 1; }
    if (fclose(fo)) { fprintf(stderr, "write to %s failed\n", pos[2]); return 1; }
    fclose(fi);
    printf("%ld frames %ldx%ld -> %ldx%ld\n", frames, w, h, w * s, h * s);
    hat_plan_free(plan);
    (void)hipFree(din);
    (void)hipFree(dout);
    free(hin);
    free(hout);
    return 0;
}
