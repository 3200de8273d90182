// rle_shape_host.h — measuring run-length masks, the host half: the checks both entries answer before a device is looked for and the
// sequential code that DEFINES the outputs of mrcnn_rle_measure and mrcnn_rle_convex_hull (the _host entries).  Plain C++17: no HIP
// header, builds with g++ alone.  One RLE at a time it cuts the runs into column pieces, sums the moments pixel by pixel, counts the
// perimeter from the pieces of neighbouring columns, and builds the hull by Andrew's monotone chain over the columns' extremes; the
// kernels of kernels_rle_shape.hip use closed forms and QuickHull and must give the same arrays.
#pragma once
#include <string>
#include <vector>

#include "rle_set_host.h"

namespace mrcnn {
namespace rle_shape {

// The flat RLE set of rle_set_host.h, nothing beside it: check_flat and check_sums there are this family's checks of the set.
using Set = rle_set::Flat;

// the hull's own arguments: null hull_offsets or n_vertices, a negative capacity, null xy with a capacity -> MRCNN_ERR_INVALID
int check_hull_arguments(const int64_t* hull_offsets, const int32_t* xy, const int64_t* n_vertices, int64_t vertex_capacity, const char* who,
                         std::string* err);
// the answer to a capacity below the hulls' vertices
int bad_capacity(long long need, long long capacity, const char* who, std::string* err);

// The definitions.  All pointers are host memory; nothing is written unless every RLE sums to its plane.
int measure_host(const Set& s, int64_t* measures, std::string* err);
// hull_offsets and *n_vertices are always written, hull_areas2 and obb (either may be null) whatever the capacity, xy only when all
// vertices fit
int convex_hull_host(const Set& s, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy, int64_t* n_vertices, int64_t vertex_capacity,
                     std::string* err);

}  // namespace rle_shape
}  // namespace mrcnn
