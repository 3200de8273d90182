// rle_combine_host.h — the set algebra of run-length masks, the host half: the checks both entries answer before a device is looked for
// and the sequential code that DEFINES the output of mrcnn_rle_combine (the _host entry).  Plain C++17: no HIP header, builds with g++
// alone.  One group at a time it decodes the first member into a plane, folds every further member into it pixel by pixel
// (combine_rule.h) and encodes; the kernel of kernels_rle_combine.hip never builds a plane and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "rle_set_host.h"

namespace mrcnn {
namespace rle_combine {

// A flat RLE set (rle_set_host.h) and the groups over it: group g combines the RLEs members[group_offsets[g] ..
// group_offsets[g+1]) in that order.  group_offsets and members are host arrays.
struct Set : rle_set::Flat {
    const int64_t* group_offsets; const int64_t* members; int64_t n_groups; int op;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers -> MRCNN_ERR_INVALID; n or
// n_groups < 0, an unknown op, a side outside 1..32767, group_offsets that do not start at 0 or decrease, an empty group, a member
// outside 0..n-1 or of another size than its group's first -> MRCNN_ERR_SHAPE (the message names the group and the member).
int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err);

// The definition.  All pointers are host memory; nothing is written unless every RLE of the set sums to its plane, out_counts only when
// all runs fit.
int combine_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err);

}  // namespace rle_combine
}  // namespace mrcnn
