// rle_components_host.h — connected components of run-length masks, the host half: the checks both entries answer before a device is
// looked for and the sequential code that DEFINES the outputs of mrcnn_rle_components and mrcnn_rle_components_select (the _host
// entries).  Plain C++17: no HIP header, builds with g++ alone.  One RLE at a time it decodes a plane and floods it from every unlabelled
// pixel in column-major order, which numbers the components as the rule orders them; the kernels of kernels_rle_components.hip never
// build a plane and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "rle_set_host.h"

namespace mrcnn {
namespace rle_components {

// A flat RLE set (rle_set_host.h) and how it is cut: the connectivity, and whether the ones or the zeros are labelled.
struct Set : rle_set::Flat {
    int connectivity; int of;
};
// the outputs of mrcnn_rle_components
struct Measures { int64_t* comp_offsets; uint32_t* comp_areas; int32_t* comp_bboxes_xywh; uint8_t* comp_flags; int64_t comp_capacity; };
// what mrcnn_rle_components_select takes and writes beyond the set
struct Select {
    const uint8_t* keep; int64_t n_comps; int mode;
    uint32_t* out_counts; int64_t capacity; int64_t* out_run_offsets; uint32_t* areas; int32_t* bboxes_xywh; int64_t* out_parent; int64_t* out_n;
};

// What can be answered without reading counts, run_offsets or keep (they may be device memory): null pointers -> MRCNN_ERR_INVALID;
// n < 0, a side outside 1..32767, a connectivity that is neither 4 nor 8, an unknown `of` or mode, SPLIT of zeros -> MRCNN_ERR_SHAPE.
int check_set(const Set& s, const char* who, std::string* err);
int check_measures(const Set& s, const Measures& m, const char* who, std::string* err);
int check_select(const Set& s, const Select& q, const char* who, std::string* err);
// the answers both entries give in the same words
int bad_comp_capacity(long long need, long long capacity, const char* who, std::string* err);
int bad_n_comps(long long given, long long found, const char* who, std::string* err);

// The definitions.  All pointers are host memory.
int components_host(const Set& s, const Measures& m, std::string* err);
int select_host(const Set& s, const Select& q, std::string* err);

}  // namespace rle_components
}  // namespace mrcnn
