// tiles_host.h — the host half of tiled prediction: the window planner, the argument checks the merge and unite entries share, and the
// sequential code that DEFINES mrcnn_merge_tiles' and mrcnn_unite_tiles' output (mrcnn_merge_tiles_host, mrcnn_unite_tiles_host).  Plain C++17: no HIP header, builds with g++
// alone.  The kernels of kernels_tiles.hip must give the same bits; the float arithmetic of the paste is restated here operation for
// operation (paste_device.h), and the translation unit is compiled without FMA contraction like the kernels.
#pragma once
#include <stddef.h>

#include "ragged.h"

namespace mrcnn {
namespace tiles {

// One merge call (the arguments of mrcnn_merge_tiles / mrcnn_merge_tiles_host, memspace aside)
struct MergeArgs {
    const float* detections; const float* masks; const mrcnn_tile* tiles;
    int n_tiles, rows, mask_size;
    const int32_t* heights; const int32_t* widths;
    int n_images, model_h, model_w;
    float threshold; int metric; double match_threshold; int max_out;
    float* detections_src; int32_t* source; int32_t* n_kept;
    uint32_t* counts; int64_t capacity; int64_t* run_offsets; uint32_t* areas; int32_t* bboxes_xywh;
    int32_t* n_parts; int32_t* group;       // mrcnn_unite_tiles only; both may be null.  There match_threshold is the link threshold.
};

// mrcnn_tile_plan.  *count is always written when the arguments are valid.
int plan(int height, int width, int tile_h, int tile_w, int overlap_y, int overlap_x, int image, mrcnn_tile* out, int capacity, int* count,
         std::string* err);

// The tile table against the images' sizes: tile.image in range, the window non-empty and inside its image (MRCNN_ERR_SHAPE; the
// message names the tile).  `who` starts the message.
int check_tiles(const mrcnn_tile* tiles, int n_tiles, const int32_t* heights, const int32_t* widths, int n_images, const char* who, std::string* err);

// Every argument check of the merge and unite entries, the per-image candidate limit included; no device is needed to answer.
// `threshold` names a.match_threshold in the message.
int check_merge(const MergeArgs& a, const char* who, std::string* err, const char* threshold = "match_threshold");

// The definition.  All pointers are host memory.
int merge_host(const MergeArgs& a, std::string* err);

// The definition of mrcnn_unite_tiles (mrcnn_unite_tiles_host): the same candidates, boxes, planes and order; linked candidates of
// different tiles become one component, whose plane is the OR of its members'.  All pointers are host memory.
int unite_host(const MergeArgs& a, std::string* err);

}  // namespace tiles
}  // namespace mrcnn
