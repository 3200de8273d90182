// components_rule.h — the connected-component rule, written once for the device and the host (include/maskrcnn_hip.h states it in
// full): which connectivity labels which value, when two set intervals of neighbouring pixel columns belong to one component, and what
// touches the border.  The host definition (rle_components_host.cpp) floods a decoded plane and shares the connectivity and the names;
// the kernels (kernels_rle_components.hip) use the interval test on the pieces of the runs.
#pragma once
#include "../../include/maskrcnn_hip.h"

#ifdef __HIPCC__
#define MRCNN_COMP_HD __host__ __device__ __forceinline__
#else
#define MRCNN_COMP_HD inline
#endif

namespace mrcnn {

// The connectivity of the labelled value: components of ones use `connectivity`, components of zeros its dual — 8 where it is 4, 4
// where it is 8 — so that a closed 4-connected ring of ones has an inside, and an 8-connected one too.
MRCNN_COMP_HD int components_connectivity(int connectivity, int of) { return of == MRCNN_COMPONENTS_OF_ONES ? connectivity : 12 - connectivity; }

// Rows [a, b) of column x and rows [c, d) of column x + 1, both of the labelled value: one component at once when they share a row
// (4) or a row or a corner (8).
MRCNN_COMP_HD bool components_meet(int a, int b, int c, int d, int conn) { return conn == 4 ? (a < d && c < b) : (a <= d && c <= b); }

// bit 0 of a component's flag: rows [a, b) of column x hold a pixel of the plane's outermost rows or columns
MRCNN_COMP_HD bool components_on_border(int x, int a, int b, int h, int w) { return x == 0 || x == w - 1 || a == 0 || b == h; }

}  // namespace mrcnn
