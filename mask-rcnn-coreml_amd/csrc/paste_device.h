// paste_device.h — the per-pixel arithmetic of the mask paste, shared by every kernel that must decide "is pixel (y, x) of row i set"
// with the paste's own bits: k_paste_masks_ragged and the RLE kernels (kernels_roialign.hip), the instance-map and render kernels
// (kernels_render.hip).  Device code only; every translation unit that includes it is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrcnn {

// One axis of the paste's bilinear sample (the set-up k_paste_masks does per y and per x): pixel i of a box that starts at `lo`,
// scale = S / the box's extent → the two mask cells it mixes and the weight of the second.  Shared by the paste and the RLE kernels:
// the same float operations in the same order (-ffp-contract=off), so both see the same bits.
struct PasteTap { int a, b; float f; };
__device__ __forceinline__ PasteTap paste_tap(int i, int lo, float scale, int S)
{
    float s = ((float)(i - lo) + 0.5f) * scale - 0.5f;
    s = fminf(fmaxf(s, 0.0f), (float)(S - 1));
    PasteTap t;
    t.a = (int)floorf(s); t.b = min(t.a + 1, S - 1);
    t.f = s - (float)t.a;
    return t;
}
// the sample itself: a, b = the upper mask row at the two columns, c, dd = the lower one
__device__ __forceinline__ float paste_lerp(float a, float b, float c, float dd, float fx, float fy)
{
    const float top = a + (b - a) * fx;
    const float bot = c + (dd - c) * fx;
    return top + (bot - top) * fy;
}

// the pixels of one row of one instance plane: what k_paste_masks derives from (instance, y) before its x loop
struct PasteRow {
    const float *ra, *rb;      // the two mask rows the bilinear sample mixes
    float fy, sx_scale;
    int x1, x2;                // columns outside [x1, x2) are 0; x1 = x2 = 0: nothing on this row
};
__device__ __forceinline__ PasteRow paste_row(const int4* __restrict__ boxes, const float* __restrict__ masks, int S, int inst, int y)
{
    PasteRow r;
    const int4 bx = boxes[inst];           // (y1, x1, y2, x2)
    r.x1 = r.x2 = 0; r.ra = r.rb = masks; r.fy = 0.f; r.sx_scale = 0.f;
    if (y >= bx.x && y < bx.z) {           // (an empty box is (0,0,0,0): no y passes)
        const float* m = masks + (size_t)inst * S * S;
        const PasteTap ty = paste_tap(y, bx.x, (float)S / (float)(bx.z - bx.x), S);
        r.fy = ty.f;
        r.ra = m + ty.a * S; r.rb = m + ty.b * S;
        r.sx_scale = (float)S / (float)(bx.w - bx.y);
        r.x1 = bx.y; r.x2 = bx.w;
    }
    return r;
}
__device__ __forceinline__ uint32_t paste_pixel(const PasteRow& r, int S, int x, float thr)
{
    if (x < r.x1 || x >= r.x2) return 0u;
    const PasteTap tx = paste_tap(x, r.x1, r.sx_scale, S);
    const float v = paste_lerp(r.ra[tx.a], r.ra[tx.b], r.rb[tx.a], r.rb[tx.b], tx.f, r.fy);
    return v >= thr ? 1u : 0u;
}

}  // namespace mrcnn
