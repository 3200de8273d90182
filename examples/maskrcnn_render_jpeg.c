/*
 * maskrcnn_render_jpeg.c — maskrcnn_render.c with the picture leaving as a file a browser opens, in plain C99 over include/maskrcnn_hip.h:
 * predict one photo and draw its detections on it (Example/Source/ViewController.swift:45-70 hands the
 * request's results to DetectionRenderer.swift:26-88).  No Python, no torch, no HIP headers.
 *
 *   config singleton → model load → mrcnn_maskrcnn_predict_images on the photo at its own size (the
 *   `.scaleFit` letterbox happens inside) → mrcnn_render_detections_source: detections with score > 0.7
 *   (Detection.swift:38), masks blended in at alpha 128/256, boxes stroked 3 pixels wide → mrcnn_jpeg_encode_batch: a baseline JPEG
 *   (quality 90, 4:2:0) encoded on the GPU, sized by the call's own size query → <out.jpg>.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_render_jpeg.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_render_jpeg
 *   ./maskrcnn_render_jpeg <artefact dir> <image.rgb> <height> <width> <out.jpg> [default|f32|f16|f32s|f32x3]
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
        fprintf(stderr, "usage: %s <artefact dir> <image.rgb> <height> <width> <out.jpg> [default|f32|f16|f32s|f32x3]\n", argc > 0 ? argv[0] : "maskrcnn_render_jpeg");
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

    const size_t n_src = (size_t)h * (size_t)w * 3u;
    uint8_t* src = (uint8_t*)malloc(n_src);
    uint8_t* out = (uint8_t*)malloc(n_src);
    float* det = (float*)malloc(sizeof(float) * (size_t)max_det * 6u);
    float* masks = (float*)malloc(sizeof(float) * (size_t)max_det * mask_size * mask_size);
    if (!src || !out || !det || !masks) { fprintf(stderr, "out of memory\n"); return 70; }
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(src, 1, n_src, f) != n_src) { fprintf(stderr, "%s: cannot read %lu bytes\n", argv[2], (unsigned long)n_src); return 66; }
    fclose(f);

    mrcnn_image image;
    image.rgb = src; image.height = h; image.width = w;
    const int64_t offset = 0;
    CHECK(mrcnn_maskrcnn_predict_images(model, &image, 1, MRCNN_HOST, det, masks));
    /* lineWidth 3 (DetectionRenderer.swift:70); the app fills opaque (alpha 256), half-transparent keeps the photo visible */
    CHECK(mrcnn_render_detections_source(&image, det, masks, 1, (int)max_det, mask_size, (int)H, (int)W, 0.5f, 0.7f, 128, 3, MRCNN_HOST, NULL, out, &offset));

    /* the rendered picture as a JPEG file: ask for the size, then encode into a buffer of exactly that size */
    mrcnn_image rendered;
    rendered.rgb = out; rendered.height = h; rendered.width = w;
    int64_t file_offsets[2] = {0, 0};
    CHECK(mrcnn_jpeg_encode_batch(&rendered, 1, MRCNN_HOST, 90, MRCNN_JPEG_420, NULL, 0, file_offsets));
    const int64_t n_file = file_offsets[1];
    uint8_t* file = (uint8_t*)malloc((size_t)n_file);
    if (!file) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(mrcnn_jpeg_encode_batch(&rendered, 1, MRCNN_HOST, 90, MRCNN_JPEG_420, file, n_file, file_offsets));

    f = fopen(argv[5], "wb");
    if (!f || fwrite(file, 1, (size_t)n_file, f) != (size_t)n_file || fclose(f) != 0) {
        fprintf(stderr, "%s: cannot write the image\n", argv[5]);
        return 73;
    }
    free(file);
    int drawn = 0;
    for (int64_t i = 0; i < max_det; ++i) drawn += det[i * 6 + 5] > 0.7f;
    printf("drawn %d\nbytes %lld\n", drawn, (long long)n_file);
    mrcnn_model_destroy(model);
    free(src); free(out); free(det); free(masks);
    return 0;
}
