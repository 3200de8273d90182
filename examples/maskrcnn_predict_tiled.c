/*
 * maskrcnn_predict_tiled.c — a large image predicted as overlapping windows, in plain C99 over include/maskrcnn_hip.h:
 *   mrcnn_tile_plan (size query, then the table) → mrcnn_maskrcnn_predict_tiles (the image crosses to the device once, the windows
 *   are never cut out) → mrcnn_merge_tiles, or mrcnn_unite_tiles with a trailing "unite" (size query, then the runs) → one line per
 *   kept detection in the image's own pixels.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_predict_tiled.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_predict_tiled
 *   ./maskrcnn_predict_tiled <artefact dir> <image.rgb> <height> <width> [overlap [iou|ios [threshold [unite]]]]
 *
 * <artefact dir> holds MaskRCNN.mrcw, Classifier.mrcw, Mask.mrcw, anchors.bin; <image.rgb> is raw interleaved RGB8 of height×width.
 * The tile is the model's input size.  Without "unite" an object is found whole only if some window holds it whole: choose the overlap
 * at least as large as the largest object of interest.  With it the threshold is the link threshold: the cut parts of an object, and
 * its duplicates, become one mask, and every line ends with the number of parts.  Exit status 0 on success; on failure the mrcnn_last_error() text goes to stderr and the
 * status code is the exit status.
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

/* the third step: the duplicates dropped (mrcnn_merge_tiles) or the parts united (mrcnn_unite_tiles) */
static int select_tiles(int unite, const float* det, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                        const int32_t* heights, const int32_t* widths, int H, int W, int metric, double threshold, int max_out, float* det_src,
                        int32_t* source, int32_t* n_kept, int32_t* n_parts, uint32_t* counts, int64_t capacity, int64_t* run_offsets,
                        uint32_t* areas, int32_t* bboxes)
{
    if (unite)
        return mrcnn_unite_tiles(det, masks, tiles, n_tiles, rows, mask_size, heights, widths, 1, H, W, 0.5f, metric, threshold, max_out, MRCNN_HOST,
                                 det_src, source, n_kept, n_parts, NULL, counts, capacity, run_offsets, areas, bboxes);
    return mrcnn_merge_tiles(det, masks, tiles, n_tiles, rows, mask_size, heights, widths, 1, H, W, 0.5f, metric, threshold, max_out, MRCNN_HOST,
                             det_src, source, n_kept, counts, capacity, run_offsets, areas, bboxes);
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s <artefact dir> <image.rgb> <height> <width> [overlap [iou|ios [threshold [unite]]]]\n", argv[0]);
        return 64;
    }
    const char* dir = argv[1];
    const int h = atoi(argv[3]), w = atoi(argv[4]);
    const int overlap = argc > 5 ? atoi(argv[5]) : 64;
    const int metric = argc > 6 && strcmp(argv[6], "iou") == 0 ? MRCNN_MATCH_IOU : MRCNN_MATCH_IOS;
    const double match_threshold = argc > 7 ? atof(argv[7]) : 0.5;
    const int unite = argc > 8 && strcmp(argv[8], "unite") == 0;
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
    if (!src) { fprintf(stderr, "out of memory\n"); return 70; }
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(src, 1, n_src, f) != n_src) { fprintf(stderr, "%s: cannot read %lu bytes\n", argv[2], (unsigned long)n_src); return 66; }
    fclose(f);

    /* the windows: the size query, then the table */
    int n_tiles = 0;
    CHECK(mrcnn_tile_plan(h, w, (int)H, (int)W, overlap, overlap, 0, NULL, 0, &n_tiles));
    mrcnn_tile* tiles = (mrcnn_tile*)malloc(sizeof(mrcnn_tile) * (size_t)n_tiles);
    float* det = (float*)malloc(sizeof(float) * (size_t)n_tiles * (size_t)rows * 6u);
    float* masks = (float*)malloc(sizeof(float) * (size_t)n_tiles * (size_t)rows * (size_t)(mask_size * mask_size));
    if (!tiles || !det || !masks) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(mrcnn_tile_plan(h, w, (int)H, (int)W, overlap, overlap, 0, tiles, n_tiles, &n_tiles));

    /* one record per window; n_tiles may exceed max_batch */
    mrcnn_image image;
    image.rgb = src; image.height = h; image.width = w;
    CHECK(mrcnn_maskrcnn_predict_tiles(model, &image, 1, tiles, n_tiles, MRCNN_HOST, det, masks));

    /* the records in the image's frame, the duplicates of the overlaps dropped or the cut parts united: the size query, then the runs */
    const int max_out = (int)rows;
    const int32_t heights[1] = {h}, widths[1] = {w};
    float* det_src = (float*)malloc(sizeof(float) * (size_t)max_out * 6u);
    int32_t* source = (int32_t*)malloc(sizeof(int32_t) * (size_t)max_out);
    int64_t* run_offsets = (int64_t*)malloc(sizeof(int64_t) * ((size_t)max_out + 1u));
    uint32_t* areas = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)max_out);
    int32_t* bboxes = (int32_t*)malloc(sizeof(int32_t) * (size_t)max_out * 4u);
    int32_t* n_parts = (int32_t*)malloc(sizeof(int32_t) * (size_t)max_out);
    int32_t n_kept = 0;
    if (!det_src || !source || !run_offsets || !areas || !bboxes || !n_parts) { fprintf(stderr, "out of memory\n"); return 70; }
    int st = select_tiles(unite, det, masks, tiles, n_tiles, (int)rows, mask_size, heights, widths, (int)H, (int)W, metric, match_threshold, max_out,
                          det_src, source, &n_kept, n_parts, NULL, 0, run_offsets, areas, bboxes);
    if (st != MRCNN_OK && st != MRCNN_ERR_SHAPE) CHECK(st);         /* MRCNN_ERR_SHAPE: the query's answer sits in run_offsets */
    const int64_t capacity = run_offsets[max_out];
    uint32_t* counts = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(capacity ? capacity : 1));
    if (!counts) { fprintf(stderr, "out of memory\n"); return 70; }
    CHECK(select_tiles(unite, det, masks, tiles, n_tiles, (int)rows, mask_size, heights, widths, (int)H, (int)W, metric, match_threshold, max_out,
                       det_src, source, &n_kept, n_parts, counts, capacity, run_offsets, areas, bboxes));

    printf("tiles %d\nkept %d\n", n_tiles, (int)n_kept);
    for (int j = 0; j < max_out && source[j] >= 0; ++j) {
        /* tile, row, class, score, tight box x y w h of the mask in the image's pixels, area, runs[, parts] */
        printf(unite ? "%d %d %d %.9g %d %d %d %d %lu %ld" : "%d %d %d %.9g %d %d %d %d %lu %ld\n", (int)(source[j] / rows), (int)(source[j] % rows), (int)det_src[j * 6 + 4],
               (double)det_src[j * 6 + 5], (int)bboxes[j * 4], (int)bboxes[j * 4 + 1], (int)bboxes[j * 4 + 2], (int)bboxes[j * 4 + 3],
               (unsigned long)areas[j], (long)(run_offsets[j + 1] - run_offsets[j]));
        if (unite) printf(" %d\n", (int)n_parts[j]);
    }
    mrcnn_model_destroy(model);
    free(src); free(tiles); free(det); free(masks); free(det_src); free(source); free(run_offsets); free(areas); free(bboxes); free(counts); free(n_parts);
    return 0;
}
