// rle_draw_host.h — drawing run-length masks, the host half: the argument checks the six entries share (the run offsets'
// and the counts' rule is rle_set_host.h's) and the sequential code that DEFINES
// the output of mrcnn_rle_decode, mrcnn_instance_map_rle and mrcnn_render_detections_rle (the _host entries).  Plain C++17: no HIP header,
// builds with g++ alone.  The kernels of kernels_rle_draw.hip must give the same bytes.  The only float arithmetic is the pixel box
// (draw_rule.h: products of a float and an int below 2^15, exact in double), shared with the kernels.
#pragma once
#include <stddef.h>

#include "ragged.h"

namespace mrcnn {
namespace rle_draw {

// An RLE set: RLE k = b*slots + i is counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[b] x widths[b] plane, column-major.
struct Set {
    const uint32_t* counts; const int64_t* run_offsets;
    int n_images, slots;
    const int32_t* heights; const int32_t* widths;
};

// What can be answered without reading counts or run_offsets (they may be device memory): null pointers and negative sizes ->
// MRCNN_ERR_INVALID, a side outside 1..32767 (ragged.h) or slots above max_slots -> MRCNN_ERR_SHAPE (the message names the image).
// The output offsets are checked by ragged.h's check_offsets.
int check_set(const Set& s, int max_slots, const char* who, std::string* err);
int check_render(int alpha, int stroke, const char* who, std::string* err);
// the answer to an RLE that does not sum to its plane (MRCNN_ERR_SHAPE naming the RLE, its image and its slot), shared with the device
// entries, which find the RLE on the device
int bad_sum(const Set& s, int64_t k, unsigned long long sum, const char* who, std::string* err);
// an RLE set in host memory: run_offsets and counts by rle_set_host.h's rule, then every RLE sums to its plane
int check_sums(const Set& s, const char* who, std::string* err);

// The definitions.  All pointers are host memory; nothing is written unless every RLE sums to its plane.
int decode_host(const Set& s, uint8_t* out, const int64_t* out_offsets, std::string* err);
int instance_map_host(const Set& s, const float* detections_src, float min_score, int16_t* map, const int64_t* map_offsets, uint32_t* visible_areas,
                      std::string* err);
int render_host(const Set& s, const mrcnn_image* images, const float* detections_src, float min_score, int alpha, int stroke, uint8_t* out_rgb,
                const int64_t* out_offsets, std::string* err);

}  // namespace rle_draw
}  // namespace mrcnn
