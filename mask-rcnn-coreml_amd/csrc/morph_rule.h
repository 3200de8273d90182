// morph_rule.h — the morphology rule, written once for the device and the host: a square structuring element of radius r on the h x w
// {0,1} plane an RLE encodes, pixels outside the image 0 for every operation (include/maskrcnn_hip.h states it in full).  The square is
// separable, and its vertical half acts on the set intervals [a, b) of one pixel column alone: that half is here, with the merging that
// has to come before it, the box the result lies in and the radius Boundary IoU takes from an image's diagonal.  The host definition
// (rle_morph_host.cpp) slides windows over a decoded plane and shares only the names and the radius; the kernels (kernels_rle_morph.hip)
// use the interval rule on the runs of a column and take the horizontal half on packed words.
#pragma once
#include <math.h>

#include "../../include/maskrcnn_hip.h"

#ifdef __HIPCC__
#define MRCNN_MORPH_HD __host__ __device__ __forceinline__
#else
#define MRCNN_MORPH_HD inline
#endif

namespace mrcnn {

struct MorphBox { int y1, x1, y2, x2; };         // y2, x2 exclusive; an empty box is (0, 0, 0, 0)

// BOUNDARY erodes like ERODE and subtracts afterwards
MRCNN_MORPH_HD bool morph_grows(int op) { return op == MRCNN_MORPH_DILATE; }

// Two set intervals of one line, [.., pb) and then [a, ..) with a >= pb, give one interval under the operation when no gap survives
// between them: erosion joins what touches (a zero-length run of zeros may lie between two runs of ones), dilation closes a gap of up
// to 2r.  Joining comes first: the halves of a touching pair would each lose r at the seam.
MRCNN_MORPH_HD bool morph_joins(int pb, int a, int r, bool grows) { return a <= pb + (grows ? 2 * r : 0); }

// The joined interval [a, b) of a line of `len` pixels under the operation: [a + r, b - r) for erosion — the line's two ends are zeros
// like any other gap — and [a - r, b + r) clipped to the line for dilation.  False: nothing is left.
MRCNN_MORPH_HD bool morph_interval(int a, int b, int r, int len, bool grows, int* oa, int* ob)
{
    if (grows) { *oa = a - r < 0 ? 0 : a - r; *ob = b + r > len ? len : b + r; }
    else { *oa = a + r; *ob = b - r; }
    return *oa < *ob;
}

// The box the result's set pixels lie in, from the tight box of the mask's own: the same for erosion, grown by r and clipped for dilation
MRCNN_MORPH_HD MorphBox morph_work_box(const MorphBox& t, int r, int h, int w, bool grows)
{
    if (!grows || (t.y2 <= t.y1 || t.x2 <= t.x1)) return t;
    MorphBox b;
    b.y1 = t.y1 - r < 0 ? 0 : t.y1 - r; b.x1 = t.x1 - r < 0 ? 0 : t.x1 - r;
    b.y2 = t.y2 + r > h ? h : t.y2 + r; b.x2 = t.x2 + r > w ? w : t.x2 + r;
    return b;
}

// r = max(1, round_half_even(ratio * sqrt(h*h + w*w))) in double: the published int(round(dilation_ratio * img_diag)) with a floor of 1
MRCNN_MORPH_HD int morph_boundary_radius(int h, int w, double ratio)
{
    const double d = rint(ratio * sqrt((double)((long long)h * h + (long long)w * w)));
    return d < 1.0 ? 1 : (d > 2147483647.0 ? 2147483647 : (int)d);
}

}  // namespace mrcnn
