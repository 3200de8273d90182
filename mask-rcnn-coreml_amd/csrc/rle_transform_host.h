// rle_transform_host.h — moving run-length masks to another pixel grid, the host half: the checks both entries answer before a device is
// looked for and the sequential code that DEFINES the output of mrcnn_rle_transform (the _host entry).  Plain C++17: no HIP header,
// builds with g++ alone.  One RLE at a time it decodes the plane, evaluates transform_rule.h's FORWARD map for every pixel of the output
// plane and encodes; it never uses the inverse.  The kernel of kernels_rle_transform.hip never builds a plane, works from the inverse
// and must give the same arrays: device against host is closed form against brute force.
#pragma once
#include <string>
#include <vector>

#include "rle_set_host.h"

namespace mrcnn {
namespace rle_transform {

// A flat RLE set (rle_set_host.h) and, per RLE, the output plane and the record: out_heights, out_widths (n) and xf (n x 8 int64)
// are host arrays.
struct Set : rle_set::Flat {
    const int32_t* out_heights; const int32_t* out_widths; const int64_t* xf;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers -> MRCNN_ERR_INVALID; n < 0,
// a side of a source or an output plane outside 1..32767, a record with an unknown flag bit, a coefficient outside its limits or a
// non-zero word 7 -> MRCNN_ERR_SHAPE (the message names the RLE).
int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err);

// The definition.  All pointers are host memory; nothing is written unless every RLE of the set sums to its plane, out_counts only when
// all runs fit.
int transform_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err);

}  // namespace rle_transform
}  // namespace mrcnn
