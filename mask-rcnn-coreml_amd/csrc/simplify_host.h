// simplify_host.h — simplifying polygon rings, the host half: the sequential code that DEFINES the output of mrcnn_polygons_simplify
// (the _host entry) and the checks both entries answer before a device is looked for.  Plain C++17: no HIP header, builds with g++
// alone.  It is classic Douglas-Peucker with an explicit stack over simplify_rule.h's distances and threshold test; the kernels of
// kernels_simplify.hip run the same chains level by level and must give the same arrays.  Integers only behind simp_tolerance.
#pragma once
#include <string>
#include <vector>

#include "ragged.h"

namespace mrcnn {
namespace simplify {

// The simplified rings (include/maskrcnn_hip.h, mrcnn_polygons_simplify): ring_offsets (n_rings + 1, in vertices), areas2 (twice the
// signed shoelace area), xy (x then y per vertex), src_index (per vertex, its index in the input xy).
struct Rings {
    std::vector<int64_t> ring_offsets, areas2, src_index;
    std::vector<int32_t> xy;
};

// What can be answered without reading ring_offsets or xy: null pointers, a negative n_rings or capacity, a tolerance that is NaN or
// outside 0..65535, null buffers with a capacity.
int check_arguments(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance, const int64_t* out_ring_offsets,
                    const int32_t* out_xy, const int64_t* n_vertices_out, int64_t vertex_capacity, const char* who, std::string* err);
// ring_offsets in host memory: they start at 0 or above, do not decrease, and no ring has 2^31 vertices or more.  *most = the largest ring.
int check_offsets(const int64_t* ring_offsets, int64_t n_rings, const char* who, std::string* err, int64_t* most);
// every coordinate of rings with such offsets lies in 0..32767 (host memory)
int check_coordinates(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, const char* who, std::string* err);
// the answers of the two content checks, shared with the device entry, which finds the ring on the device
int bad_offsets(int64_t ring, const char* who, std::string* err);
int bad_coordinate(int64_t ring, const char* who, std::string* err);
// the simplified vertices fit the caller's buffers, or MRCNN_ERR_SHAPE naming the size needed
int check_capacity(int64_t vertices, int64_t vertex_capacity, const char* who, std::string* err);

// The definition.  All pointers are host memory and have passed the checks above; E = simp_tolerance(tolerance).
void simplify_host(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, uint64_t E, Rings* out);

}  // namespace simplify
}  // namespace mrcnn
