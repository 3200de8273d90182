/*
 * maskrcnn_instance_png.c — the label image of a predict as a file an annotation tool opens, in plain C99 over include/maskrcnn_hip.h:
 * predict one photo and write which detection owns each pixel.  No Python, no torch, no HIP headers, no codec.
 *
 *   config singleton → model load → mrcnn_maskrcnn_predict_images on the photo at its own size (the
 *   `.scaleFit` letterbox happens inside) → mrcnn_instance_map_source: the int16 map, the lowest row whose mask (threshold 0.5)
 *   covers the pixel, -1 where there is none → mrcnn_png_encode_batch: an 8-bit palette PNG (index = row + 1, index 0
 *   transparent, the colours of maskrcnn_render.c) whose deflate stream is made on the GPU, sized by the call's own size
 *   query → <out.png>.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_instance_png.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_instance_png
 *   ./maskrcnn_instance_png <artefact dir> <image.rgb> <height> <width> <out.png> [default|f32|f16|f32s|f32x3]
 *
 * <artefact dir> holds MaskRCNN.mrcw, Classifier.mrcw, Mask.mrcw, anchors.bin; <image.rgb> is raw
 * interleaved RGB8 of height×width.  Exit status 0 on success; on failure the mrcnn_last_error()
 * text goes to stderr and the status code is the exit status.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "maskrcnn_hip.h"

#define CHECK(call)                                                                          \
    do {                                                                                     \
        int st_ = (call);                                                                    \
        if (st_ != MRCNN_OK) {                                                               \
            fprintf(stderr, "%s failed (%d): %s\n", #call, st_, mrcnn_last_error());         \
            return st_;                                                                      \
        }                                                                                    \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 6) {
        fprintf(stderr, "usage: %s <artefact dir> <image.rgb> <height> <width> <out.png> [default|f32|f16|f32s|f32x3]\n", argc > 0 ? argv[0] : "maskrcnn_instance_png");
        return 64;
    }
    const char* dir = argv[1];
    const int h = atoi(argv[3]), w = atoi(argv[4]);
    const int dtype = argc <= 6 || strcmp(argv[6], "default") == 0 ? MRCNN_DEFAULT : strcmp(argv[6], "f16") == 0 ? MRCNN_F16 : strcmp(argv[6], "f32s") == 0 ? MRCNN_F32S
                    : strcmp(argv[6], "f32x3") == 0 ? MRCNN_F32X3 : MRCNN_F32;
    if (h < 1 || w < 1 || h > 32767 || w > 32767) { fprintf(stderr, "height and width must lie in 1..32767\n"); return 64; }
    char path[4][4096];
    snprintf(path[0], sizeof path[0], "%s/anchors.bin", dir);
    snprintf(path[1], sizeof path[1], "%s/Classifier.mrcw", dir);
    snprintf(path[2], sizeof path[2], "%s/Mask.mrcw", dir);
    snprintf(path[3], sizeof path[3], "%s/MaskRCNN.mrcw", dir);

    /* MaskRCNNConfig.defaultConfig must be set before the model is created (AppDelegate.swift:18-20) */
    CHECK(mrcnn_config_set_anchors_path(path[0]));
    CHECK(mrcnn_config_set_classifier_path(path[1]));
    CHECK(mrcnn_config_set_mask_path(path[2]));
    mrcnn_model* model = NULL;
    CHECK(mrcnn_model_load(MRCNN_MODEL_MASKRCNN, path[3], 1, dtype, &model));

    int64_t H = 0, W = 0, max_det = 0;
    CHECK(mrcnn_model_get_int(model, "image_height", &H));
    CHECK(mrcnn_model_get_int(model, "image_width", &W));
    CHECK(mrcnn_model_get_int(model, "max_detections", &max_det));
    const int mask_size = 28;
    if (max_det > 255) { fprintf(stderr, "max_detections %ld: an 8-bit palette file holds 255 rows\n", (long)max_det); return 64; }

    const size_t n_pixels = (size_t)h * (size_t)w;
    uint8_t* src = (uint8_t*)malloc(n_pixels * 3u);
    int16_t* map = (int16_t*)malloc(n_pixels * sizeof(int16_t));
    float* det = (float*)malloc(sizeof(float) * (size_t)max_det * 6u);
    float* det_src = (float*)malloc(sizeof(float) * (size_t)max_det * 6u);
    float* masks = (float*)malloc(sizeof(float) * (size_t)max_det * mask_size * mask_size);
    if (!src || !map || !det || !det_src || !masks) { fprintf(stderr, "out of memory\n"); return 70; }
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(src, 1, n_pixels * 3u, f) != n_pixels * 3u) { fprintf(stderr, "%s: cannot read %lu bytes\n", argv[2], (unsigned long)(n_pixels * 3u)); return 66; }
    fclose(f);

    mrcnn_image image;
    image.rgb = src; image.height = h; image.width = w;
    const int32_t height = h, width = w;
    const int64_t offset = 0;
    CHECK(mrcnn_maskrcnn_predict_images(model, &image, 1, MRCNN_HOST, det, masks));
    /* every detection with a score above 0 owns its pixels; the most confident wins a contested one */
    CHECK(mrcnn_instance_map_source(det, masks, 1, (int)max_det, mask_size, &height, &width, (int)H, (int)W, 0.5f, 0.0f, MRCNN_HOST, det_src, map, &offset, NULL));

    /* the map as a PNG file: ask for the size, then encode into a buffer of exactly that size */
    mrcnn_png_source label;
    label.pixels = map; label.height = h; label.width = w;
    int64_t file_offsets[2] = {0, 0};
    CHECK(mrcnn_png_encode_batch(&label, 1, MRCNN_HOST, MRCNN_PNG_INSTANCE, (int)max_det, NULL, 0, file_offsets));
    const int64_t n_file = file_offsets[1];
    uint8_t* file = (uint8_t*)malloc((size_t)n_file);
    if (!file) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(mrcnn_png_encode_batch(&label, 1, MRCNN_HOST, MRCNN_PNG_INSTANCE, (int)max_det, file, n_file, file_offsets));

    f = fopen(argv[5], "wb");
    if (!f || fwrite(file, 1, (size_t)n_file, f) != (size_t)n_file || fclose(f) != 0) {
        fprintf(stderr, "%s: cannot write the image\n", argv[5]);
        return 73;
    }
    free(file);
    int instances = 0;
    for (int64_t i = 0; i < max_det; ++i) instances += det[i * 6 + 5] > 0.0f;
    printf("instances %d\nbytes %lld\n", instances, (long long)n_file);
    mrcnn_model_destroy(model);
    free(src); free(map); free(det); free(det_src); free(masks);
    return 0;
}
