// rle_morph_host.h — morphology on run-length masks, the host half: the checks both entries answer before a device is looked for and the
// sequential code that DEFINES the output of mrcnn_rle_morph (the _host entry).  Plain C++17: no HIP header, builds with g++ alone.  One
// RLE at a time it decodes a plane, runs the two halves of the square as sliding windows over running counts — O(h*w) whatever the
// radius — and encodes the result; the kernels of kernels_rle_morph.hip never build a plane and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "rle_set_host.h"

namespace mrcnn {
namespace rle_morph {

// A flat RLE set (rle_set_host.h) and what is done to it: radii[k] is RLE k's radius, a host array of n.
struct Set : rle_set::Flat {
    const int32_t* radii; int op;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers -> MRCNN_ERR_INVALID; n < 0,
// a side outside 1..32767, a radius outside 0..MRCNN_MORPH_MAX_RADIUS, an unknown op -> MRCNN_ERR_SHAPE (the message names the RLE).
int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err);

// The definition.  All pointers are host memory and have passed check_arguments; nothing is written unless every RLE sums to its plane,
// out_counts only when all runs fit.
int morph_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err);

}  // namespace rle_morph
}  // namespace mrcnn
