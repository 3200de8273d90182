// polygons_host.h — run-length masks to polygon rings, the host half: the sequential code that DEFINES the output of
// mrcnn_rle_to_polygons (the _host entry).  Plain C++17: no HIP header, builds with g++ alone.  It decodes a plane and walks its directed
// unit edges one by one with polygon_rule.h's turn rule; the kernels of kernels_polygons.hip never see a pixel and must give the same
// arrays.  Integers only.
#pragma once
#include <vector>

#include "rle_draw_host.h"

namespace mrcnn {
namespace polygons {

// The rings of an RLE set (include/maskrcnn_hip.h, mrcnn_rle_to_polygons): rle_rings (n + 1), ring_offsets (rings + 1, in vertices),
// ring_areas (rings, signed), xy (x then y per vertex).
struct Rings {
    std::vector<int64_t> rle_rings, ring_offsets, ring_areas;
    std::vector<int32_t> xy;
};

// What can be answered without reading counts or run_offsets: rle_draw::check_set's answers, null outputs and bad capacities.
int check_arguments(const rle_draw::Set& s, const int64_t* rle_rings, const int64_t* n_rings, const int64_t* n_vertices, const int64_t* ring_offsets,
                    int64_t ring_capacity, const int32_t* xy, int64_t vertex_capacity, const char* who, std::string* err);
// rings and vertices fit the caller's buffers, or MRCNN_ERR_SHAPE naming both sizes needed
int check_capacity(int64_t rings, int64_t vertices, int64_t ring_capacity, int64_t vertex_capacity, const char* who, std::string* err);

// The definition.  All pointers are host memory; `out` is untouched unless every RLE sums to its plane.
int trace_host(const rle_draw::Set& s, const char* who, Rings* out, std::string* err);

}  // namespace polygons
}  // namespace mrcnn
