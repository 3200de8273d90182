// nest_host.h — nesting polygon rings into outlines and their holes, the host half: the sequential code that DEFINES the output of
// mrcnn_polygons_nest (the _host entry) and the checks both entries answer before a device is looked for.  Plain C++17: no HIP header,
// builds with g++ alone.  Per ring it loops over the other rings of the RLE and over their edges with nest_rule.h's crossing test; the
// kernels of kernels_nest.hip split the same loops over workgroups, waves and lanes and must give the same arrays.  The checks of
// ring_offsets and xy are simplify_host.h's: the two entries take the same rings.
#pragma once
#include <string>
#include <vector>

#include "ragged.h"

namespace mrcnn {
namespace nest {

// The nesting (include/maskrcnn_hip.h, mrcnn_polygons_nest): parent and depth per ring, rle_polys (n_rles + 1), poly_rings
// (n_polys + 1), ring_order (a permutation of the rings).
struct Nest {
    std::vector<int64_t> parent, rle_polys, poly_rings, ring_order;
    std::vector<int32_t> depth;
};

// What can be answered without reading an array: null pointers, negative counts.
int check_arguments(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, const int64_t* parent,
                    const int32_t* depth, const int64_t* rle_polys, const int64_t* poly_rings, const int64_t* ring_order, const int64_t* n_polys,
                    const char* who, std::string* err);
// rle_rings in host memory: it starts at 0, does not decrease and ends at n_rings
int check_rle_rings(const int64_t* rle_rings, int64_t n_rles, int64_t n_rings, const char* who, std::string* err);
// the answer of that check, shared with the device entry, which finds the RLE on the device
int bad_rle_rings(int64_t rle, int64_t n_rings, const char* who, std::string* err);

// The definition.  All pointers are host memory and have passed the checks above and simplify_host.h's two.
void nest_host(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, Nest* out);

}  // namespace nest
}  // namespace mrcnn
