// combine_rule.h — the set algebra of run-length masks, written once for the device and the host (include/maskrcnn_hip.h states it in
// full): the members of a group, all of one plane size, are folded from the first one on, bit by bit.  The fold acts on any number of
// bits at once: the host definition (rle_combine_host.cpp) folds the bytes of decoded planes, the kernel (kernels_rle_combine.hip) folds
// the runs of a pixel column into the 32-row words of a packed bit box and never builds a plane.  Also here: the box the result lies in.
#pragma once
#include <stdint.h>

#include "morph_rule.h"

#ifdef __HIPCC__
#define MRCNN_COMBINE_HD __host__ __device__ __forceinline__
#else
#define MRCNN_COMBINE_HD inline
#endif

namespace mrcnn {

MRCNN_COMBINE_HD bool combine_known(int op) { return op == MRCNN_RLE_OR || op == MRCNN_RLE_AND || op == MRCNN_RLE_XOR || op == MRCNN_RLE_DIFF; }

// the bits `acc` of the members folded so far and the bits `m` of the next member: a member listed twice is folded twice, so XOR counts
// parity and DIFF by the first member itself is empty
template <class T>
MRCNN_COMBINE_HD T combine_fold(int op, T acc, T m)
{
    switch (op) {
    case MRCNN_RLE_OR: return (T)(acc | m);
    case MRCNN_RLE_AND: return (T)(acc & m);
    case MRCNN_RLE_XOR: return (T)(acc ^ m);
    default: return (T)(acc & (T)~m);                        // MRCNN_RLE_DIFF
    }
}

// AND and DIFF only clear pixels of the first member: their result lies in its tight box; OR and XOR need the hull of all members'
MRCNN_COMBINE_HD bool combine_in_first(int op) { return op == MRCNN_RLE_AND || op == MRCNN_RLE_DIFF; }

// the smallest box around two tight boxes; an empty box (y2 <= y1 or x2 <= x1) adds nothing
MRCNN_COMBINE_HD MorphBox combine_hull(const MorphBox& a, const MorphBox& b)
{
    if (a.y2 <= a.y1 || a.x2 <= a.x1) return b;
    if (b.y2 <= b.y1 || b.x2 <= b.x1) return a;
    MorphBox o;
    o.y1 = a.y1 < b.y1 ? a.y1 : b.y1; o.x1 = a.x1 < b.x1 ? a.x1 : b.x1;
    o.y2 = a.y2 > b.y2 ? a.y2 : b.y2; o.x2 = a.x2 > b.x2 ? a.x2 : b.x2;
    return o;
}

}  // namespace mrcnn
