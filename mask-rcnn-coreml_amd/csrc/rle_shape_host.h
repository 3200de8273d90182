// rle_shape_host.h — measuring run-length masks, the host half: the checks both entries answer before a device is looked for and the
// sequential code that DEFINES the outputs of mrcnn_rle_measure and mrcnn_rle_convex_hull (the _host entries).  Plain C++17: no HIP
// header, builds with g++ alone.  One RLE at a time it cuts the runs into column pieces, sums the moments pixel by pixel, counts the
// perimeter from the pieces of neighbouring columns, and builds the hull by Andrew's monotone chain over the columns' extremes; the
// kernels of kernels_rle_shape.hip use closed forms and QuickHull and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "ragged.h"

namespace mrcnn {
namespace rle_shape {

// A flat RLE set as rle_morph_host.h takes it.  heights and widths are host arrays of n.
struct Set {
    const uint32_t* counts; const int64_t* run_offsets; int64_t n;
    const int32_t* heights; const int32_t* widths;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers -> MRCNN_ERR_INVALID; n < 0,
// a side outside 1..32767 -> MRCNN_ERR_SHAPE (the message names the RLE).
int check_set(const Set& s, const char* who, std::string* err);
// the hull's own arguments: null hull_offsets or n_vertices, a negative capacity, null xy with a capacity -> MRCNN_ERR_INVALID
int check_hull_arguments(const int64_t* hull_offsets, const int32_t* xy, const int64_t* n_vertices, int64_t vertex_capacity, const char* who,
                         std::string* err);
// the answer to an RLE that does not sum to its plane, shared with the device entries, which find the RLE on the device
int bad_sum(const Set& s, int64_t k, unsigned long long sum, const char* who, std::string* err);
// the answer to a capacity below the hulls' vertices
int bad_capacity(long long need, long long capacity, const char* who, std::string* err);
// an RLE set in host memory: run_offsets do not decrease, every RLE sums to its plane (the lowest k that does not is named)
int check_sums(const Set& s, const char* who, std::string* err);

// The definitions.  All pointers are host memory; nothing is written unless every RLE sums to its plane.
int measure_host(const Set& s, int64_t* measures, std::string* err);
// hull_offsets and *n_vertices are always written, hull_areas2 and obb (either may be null) whatever the capacity, xy only when all
// vertices fit
int convex_hull_host(const Set& s, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy, int64_t* n_vertices, int64_t vertex_capacity,
                     std::string* err);

}  // namespace rle_shape
}  // namespace mrcnn
