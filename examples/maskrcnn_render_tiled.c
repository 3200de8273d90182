/*
 * maskrcnn_render_tiled.c — a large image predicted as overlapping windows, the cut parts united, and the result DRAWN, in plain C99
 * over include/maskrcnn_hip.h:
 *   mrcnn_tile_plan → mrcnn_maskrcnn_predict_tiles → mrcnn_unite_tiles (size query, then the runs) → mrcnn_render_detections_rle: the
 *   united masks blended in at alpha 128/256 straight from their run lengths, the boxes stroked 3 pixels wide, rows with score > 0.7 →
 *   mrcnn_jpeg_encode_batch (quality 90, 4:2:0, sized by its own size query) → <out.jpg>.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_render_tiled.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_render_tiled
 *   ./maskrcnn_render_tiled <artefact dir> <image.rgb> <height> <width> <out.jpg> [overlap [link threshold]]
 *
 * <artefact dir> holds MaskRCNN.mrcw, Classifier.mrcw, Mask.mrcw, anchors.bin; <image.rgb> is raw interleaved RGB8 of height×width.
 * The tile is the model's input size.  Exit status 0 on success; on failure the mrcnn_last_error() text goes to stderr and the status
 * code is the exit status.
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
        fprintf(stderr, "usage: %s <artefact dir> <image.rgb> <height> <width> <out.jpg> [overlap [link threshold]]\n", argv[0]);
        return 64;
    }
    const char* dir = argv[1];
    const int h = atoi(argv[3]), w = atoi(argv[4]);
    const int overlap = argc > 6 ? atoi(argv[6]) : 64;
    const double link_threshold = argc > 7 ? atof(argv[7]) : 0.5;
    const int max_batch = 4, mask_size = 28;
    char path[4][4096];
    snprintf(path[0], sizeof path[0], "%s/anchors.bin", dir);
    snprintf(path[1], sizeof path[1], "%s/Classifier.mrcw", dir);
    snprintf(path[2], sizeof path[2], "%s/Mask.mrcw", dir);
    snprintf(path[3], sizeof path[3], "%s/MaskRCNN.mrcw", dir);
    CHECK(mrcnn_config_set_anchors_path(path[0]));
    CHECK(mrcnn_config_set_classifier_path(path[1]));
    CHECK(mrcnn_config_set_mask_path(path[2]));
    mrcnn_model* model = NULL;
    CHECK(mrcnn_model_load(MRCNN_MODEL_MASKRCNN, path[3], max_batch, MRCNN_DEFAULT, &model));
    int64_t H = 0, W = 0, rows = 0;
    CHECK(mrcnn_model_get_int(model, "image_height", &H));
    CHECK(mrcnn_model_get_int(model, "image_width", &W));
    CHECK(mrcnn_model_get_int(model, "max_detections", &rows));

    const size_t n_src = (size_t)h * (size_t)w * 3u;
    uint8_t* src = (uint8_t*)malloc(n_src ? n_src : 1);
    uint8_t* out = (uint8_t*)malloc(n_src ? n_src : 1);
    if (!src || !out) { fprintf(stderr, "out of memory\n"); return 70; }
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(src, 1, n_src, f) != n_src) { fprintf(stderr, "%s: cannot read %lu bytes\n", argv[2], (unsigned long)n_src); return 66; }
    fclose(f);

    /* the windows and one record per window */
    int n_tiles = 0;
    CHECK(mrcnn_tile_plan(h, w, (int)H, (int)W, overlap, overlap, 0, NULL, 0, &n_tiles));
    mrcnn_tile* tiles = (mrcnn_tile*)malloc(sizeof(mrcnn_tile) * (size_t)n_tiles);
    float* det = (float*)malloc(sizeof(float) * (size_t)n_tiles * (size_t)rows * 6u);
    float* masks = (float*)malloc(sizeof(float) * (size_t)n_tiles * (size_t)rows * (size_t)(mask_size * mask_size));
    if (!tiles || !det || !masks) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(mrcnn_tile_plan(h, w, (int)H, (int)W, overlap, overlap, 0, tiles, n_tiles, &n_tiles));
    mrcnn_image image;
    image.rgb = src; image.height = h; image.width = w;
    CHECK(mrcnn_maskrcnn_predict_tiles(model, &image, 1, tiles, n_tiles, MRCNN_HOST, det, masks));

    /* the cut parts united: the size query, then the runs */
    const int max_out = (int)rows;
    const int32_t heights[1] = {h}, widths[1] = {w};
    float* det_src = (float*)malloc(sizeof(float) * (size_t)max_out * 6u);
    int32_t* source = (int32_t*)malloc(sizeof(int32_t) * (size_t)max_out);
    int64_t* run_offsets = (int64_t*)malloc(sizeof(int64_t) * ((size_t)max_out + 1u));
    int32_t n_kept = 0;
    if (!det_src || !source || !run_offsets) { fprintf(stderr, "out of memory\n"); return 70; }
    int st = mrcnn_unite_tiles(det, masks, tiles, n_tiles, (int)rows, mask_size, heights, widths, 1, (int)H, (int)W, 0.5f, MRCNN_MATCH_IOU, link_threshold,
                               max_out, MRCNN_HOST, det_src, source, &n_kept, NULL, NULL, NULL, 0, run_offsets, NULL, NULL);
    if (st != MRCNN_OK && st != MRCNN_ERR_SHAPE) CHECK(st);         /* MRCNN_ERR_SHAPE: the query's answer sits in run_offsets */
    const int64_t capacity = run_offsets[max_out];
    uint32_t* counts = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(capacity ? capacity : 1));
    if (!counts) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(mrcnn_unite_tiles(det, masks, tiles, n_tiles, (int)rows, mask_size, heights, widths, 1, (int)H, (int)W, 0.5f, MRCNN_MATCH_IOU, link_threshold,
                            max_out, MRCNN_HOST, det_src, source, &n_kept, NULL, NULL, counts, capacity, run_offsets, NULL, NULL));

    /* the overlay from the run lengths: no 28x28 mask reproduces a united mask */
    const int64_t out_offsets[1] = {0};
    CHECK(mrcnn_render_detections_rle(&image, det_src, counts, run_offsets, 1, max_out, 0.7f, 128, 3, MRCNN_HOST, out, out_offsets));

    /* the file: the size query, then the bytes */
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
    printf("tiles %d\nunited %d\n%s %ld bytes\n", n_tiles, (int)n_kept, argv[5], (long)n_file);
    mrcnn_model_destroy(model);
    free(src); free(out); free(tiles); free(det); free(masks); free(det_src); free(source); free(run_offsets); free(counts); free(file);
    return 0;
}
