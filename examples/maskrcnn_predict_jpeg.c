/*
 * maskrcnn_predict_jpeg.c — maskrcnn_predict.c for photos: JPEG files in, detections out, in plain C99 over
 * include/maskrcnn_hip.h with no size arguments and no codec linked.  The files are read as bytes; their entropy
 * decoders run on this host's threads, everything after them — inverse DCT, chroma upsampling, colour
 * conversion, the letterbox and the network — on the GPU (mrcnn_maskrcnn_predict_jpegs), all files in ONE batch.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_predict_jpeg.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_predict_jpeg
 *   ./maskrcnn_predict_jpeg <artefact dir> <file.jpg> [more.jpg ...] [device-entropy]
 *
 * A trailing word `device-entropy` decodes the Huffman streams on the GPU as well (mrcnn_maskrcnn_predict_jpegs_on with
 * MRCNN_JPEG_ENTROPY_DEVICE, opt-in): the output is the same.
 *
 * Prints `seconds`, then per file `image <k> <height> <width> detections <n>` and one line per detection with
 * score > 0.7: row, class, score, the box normalized in the letterboxed frame (mrcnn_unletterbox_boxes maps it
 * to the file's own pixels), mask checksum.  Exit status 0 on success; on failure the mrcnn_last_error() text
 * goes to stderr and the status code is the exit status.
 */
#define _POSIX_C_SOURCE 200809L   /* clock_gettime under -std=c99 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "maskrcnn_hip.h"

#define CHECK(call)                                                                          \
    do {                                                                                     \
        int st_ = (call);                                                                    \
        if (st_ != MRCNN_OK) {                                                               \
            fprintf(stderr, "%s failed (%d): %s\n", #call, st_, mrcnn_last_error());         \
            return st_;                                                                      \
        }                                                                                    \
    } while (0)

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int read_file(const char* path, mrcnn_jpeg* out)
{
    FILE* f = fopen(path, "rb");
    long n;
    uint8_t* p;
    if (!f) return 0;
    if (fseek(f, 0, SEEK_END) != 0 || (n = ftell(f)) <= 0 || fseek(f, 0, SEEK_SET) != 0) { fclose(f); return 0; }
    p = (uint8_t*)malloc((size_t)n);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(p); return 0; }
    fclose(f);
    out->data = p;
    out->length = (int64_t)n;
    return 1;
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s <artefact dir> <file.jpg> [more.jpg ...]\n", argv[0]);
        return 64;
    }
    const char* dir = argv[1];
    const int entropy = argc > 3 && strcmp(argv[argc - 1], "device-entropy") == 0 ? MRCNN_JPEG_ENTROPY_DEVICE : MRCNN_JPEG_ENTROPY_HOST;
    const int batch = argc - 2 - (entropy == MRCNN_JPEG_ENTROPY_DEVICE ? 1 : 0);
    const int mask_size = 28;
    char path[4][4096];
    snprintf(path[0], sizeof path[0], "%s/anchors.bin", dir);
    snprintf(path[1], sizeof path[1], "%s/Classifier.mrcw", dir);
    snprintf(path[2], sizeof path[2], "%s/Mask.mrcw", dir);
    snprintf(path[3], sizeof path[3], "%s/MaskRCNN.mrcw", dir);

    mrcnn_jpeg* files = (mrcnn_jpeg*)calloc((size_t)batch, sizeof(mrcnn_jpeg));
    int32_t* heights = (int32_t*)calloc((size_t)batch, sizeof(int32_t));
    int32_t* widths = (int32_t*)calloc((size_t)batch, sizeof(int32_t));
    if (!files || !heights || !widths) { fprintf(stderr, "out of memory\n"); return 70; }
    for (int b = 0; b < batch; ++b) {
        int32_t comps = 0, hs = 0, vs = 0;
        if (!read_file(argv[2 + b], &files[b])) { fprintf(stderr, "%s: cannot read\n", argv[2 + b]); return 66; }
        /* host code, no GPU: a file the decoder does not take is named here, before the model is loaded */
        CHECK(mrcnn_jpeg_info(files[b].data, files[b].length, &heights[b], &widths[b], &comps, &hs, &vs));
    }

    CHECK(mrcnn_config_set_anchors_path(path[0]));
    CHECK(mrcnn_config_set_classifier_path(path[1]));
    CHECK(mrcnn_config_set_mask_path(path[2]));
    mrcnn_model* model = NULL;
    CHECK(mrcnn_model_load(MRCNN_MODEL_MASKRCNN, path[3], batch, MRCNN_DEFAULT, &model));
    int64_t max_det = 0;
    CHECK(mrcnn_model_get_int(model, "max_detections", &max_det));

    float* det = (float*)malloc(sizeof(float) * (size_t)batch * (size_t)max_det * 6u);
    float* masks = (float*)malloc(sizeof(float) * (size_t)batch * (size_t)max_det * mask_size * mask_size);
    mrcnn_detection* recs = (mrcnn_detection*)malloc(sizeof(mrcnn_detection) * (size_t)max_det);
    if (!det || !masks || !recs) { fprintf(stderr, "out of memory\n"); return 70; }

    const double t0 = now_s();
    CHECK(mrcnn_maskrcnn_predict_jpegs_on(model, files, batch, MRCNN_HOST, entropy, det, masks, heights, widths));
    const double t1 = now_s();

    printf("seconds %.6f\n", t1 - t0);
    for (int b = 0; b < batch; ++b) {
        int64_t n = 0;
        const float* mb = masks + (size_t)b * (size_t)max_det * mask_size * mask_size;
        CHECK(mrcnn_detections_decode(det + (size_t)b * (size_t)max_det * 6u, max_det, 6, recs, max_det, &n));
        printf("image %d %d %d detections %lld\n", b, (int)heights[b], (int)widths[b], (long long)n);
        for (int64_t i = 0; i < n; ++i) {
            const float* m = mb + (size_t)recs[i].index * mask_size * mask_size;
            double sum = 0.0;
            for (int k = 0; k < mask_size * mask_size; ++k) sum += (double)m[k];
            printf("%lld %lld %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)recs[i].index, (long long)recs[i].class_id,
                   recs[i].score, recs[i].x, recs[i].y, recs[i].w, recs[i].h, sum);
        }
    }
    mrcnn_model_destroy(model);
    for (int b = 0; b < batch; ++b) free((void*)files[b].data);
    free(files); free(heights); free(widths); free(det); free(masks); free(recs);
    return 0;
}
