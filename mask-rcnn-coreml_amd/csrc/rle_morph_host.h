// rle_morph_host.h — morphology on run-length masks, the host half: the checks both entries answer before a device is looked for and the
// sequential code that DEFINES the output of mrcnn_rle_morph (the _host entry).  Plain C++17: no HIP header, builds with g++ alone.  One
// RLE at a time it decodes a plane, runs the two halves of the square as sliding windows over running counts — O(h*w) whatever the
// radius — and encodes the result; the kernels of kernels_rle_morph.hip never build a plane and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "ragged.h"

namespace mrcnn {
namespace rle_morph {

// A flat RLE set: RLE k is counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane, column-major;
// radii[k] is its radius.  heights, widths and radii are host arrays of n.
struct Set {
    const uint32_t* counts; const int64_t* run_offsets; int64_t n;
    const int32_t* heights; const int32_t* widths; const int32_t* radii; int op;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers -> MRCNN_ERR_INVALID; n < 0,
// a side outside 1..32767, a radius outside 0..MRCNN_MORPH_MAX_RADIUS, an unknown op -> MRCNN_ERR_SHAPE (the message names the RLE).
int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err);
// the answer to an RLE that does not sum to its plane, shared with the device entry, which finds the RLE on the device
int bad_sum(const Set& s, int64_t k, unsigned long long sum, const char* who, std::string* err);
// the answer to a capacity below the runs of the result
int bad_capacity(long long need, long long capacity, const char* who, std::string* err);
// an RLE set in host memory: run_offsets do not decrease, every RLE sums to its plane (the lowest k that does not is named)
int check_sums(const Set& s, const char* who, std::string* err);

// The definition.  All pointers are host memory and have passed check_arguments; nothing is written unless every RLE sums to its plane,
// out_counts only when all runs fit.
int morph_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err);

}  // namespace rle_morph
}  // namespace mrcnn
