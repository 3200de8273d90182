// rle_device.h — the walk of the COCO run-length kernels, shared by k_rle_count / k_rle_write (kernels_roialign.hip: one pasted mask
// per plane) and the union encoder of kernels_tiles.hip (the OR of several pasted masks per plane).  kernels_roialign.hip explains the
// scheme: the columns of a box cut into chunks of 63 consecutive positions, one wave per chunk, transitions from one ballot.
#pragma once
#include "kernels.h"
#include "paste_device.h"

namespace mrcnn {

// the paste's bit of pixel (y, x) for the mask m pasted into box bx of a plane of height h; y = -1 / y = h name the position before a
// column's first / behind its last pixel
__device__ __forceinline__ bool rle_bit(const int4 bx, const float* __restrict__ m, int S, int h, int x, int y, float thr)
{
    if (y < 0) { --x; y = h - 1; } else if (y >= h) { ++x; y = 0; }        // the position before a column's first / behind its last pixel
    if (x < bx.y || x >= bx.w || y < bx.x || y >= bx.z) return false;
    const PasteTap ty = paste_tap(y, bx.x, (float)S / (float)(bx.z - bx.x), S);
    const PasteTap tx = paste_tap(x, bx.y, (float)S / (float)(bx.w - bx.y), S);
    const float *ra = m + ty.a * S, *rb = m + ty.b * S;
    return paste_lerp(ra[tx.a], ra[tx.b], rb[tx.a], rb[tx.b], tx.f, ty.f) >= thr;
}

// One chunk: lane l stands for position p0 + l (p0 may be "-1" for the chunk that starts the plane: lane 0 is never a candidate).
struct RleChunk {
    unsigned long long set;     // candidate lanes whose pixel is 1 (every pixel of the box is a candidate of exactly one chunk)
    unsigned long long trans;   // candidate lanes that are transitions
    uint32_t p0;
    int x, y0;                  // lane l: column x, row y0 + l
};
struct RleWalk {
    int4 bx; const float* m; int S, h, w, nchunk; long items; float thr;
};
// the chunks of box k.bx in a plane of k.h x k.w (no set pixel lies outside the box)
__device__ __forceinline__ void rle_walk_box(RleWalk& k)
{
    k.nchunk = (k.bx.z - k.bx.x + 1 + 62) / 63;                            // candidates per column: rows y1 .. y2 (y2 = the position behind)
    k.items = (long)(k.bx.w - k.bx.y) * k.nchunk;                          // (an empty box is (0,0,0,0): no items)
}
__device__ __forceinline__ RleWalk rle_walk(const ImageGeom* __restrict__ tab, const int4* __restrict__ boxes, const float* __restrict__ masks,
                                            int rows, int S, float thr, int inst)
{
    RleWalk k;
    const ImageGeom im = tab[inst / rows];
    k.bx = boxes[inst]; k.m = masks + (size_t)inst * S * S; k.S = S; k.h = im.h; k.w = im.w; k.thr = thr;
    rle_walk_box(k);
    return k;
}
// bit(x, y): the plane's pixel, y = -1 / y = h as rle_bit takes them
template <class Bit>
__device__ __forceinline__ RleChunk rle_chunk_of(const RleWalk& k, long item, int lane, Bit bit)
{
    RleChunk c;
    c.x = k.bx.y + (int)(item / k.nchunk);
    c.y0 = k.bx.x - 1 + 63 * (int)(item % k.nchunk);
    const int y = c.y0 + lane;
    // the last candidate of this column: the position behind the box's last row — unless that position is the first candidate of the
    // next column (a box of the plane's full height) or lies behind the plane's end (no transition there: the last run just ends)
    int hi = k.bx.z;
    if (k.bx.z == k.h && ((k.bx.x == 0 && c.x < k.bx.w - 1) || c.x == k.w - 1)) hi = k.h - 1;
    const bool valid = y <= hi;
    const bool cur = valid && bit(c.x, y);
    const unsigned long long bal = __ballot(cur);
    const unsigned long long cand = __ballot(valid && lane >= 1);
    c.set = bal & cand;
    c.trans = (bal ^ (bal << 1)) & cand;
    c.p0 = (uint32_t)c.x * (uint32_t)k.h + (uint32_t)c.y0;
    return c;
}
// the bit of the one mask k.m pasted into k.bx
struct RleOneMask {
    const RleWalk& k;
    __device__ __forceinline__ bool operator()(int x, int y) const { return rle_bit(k.bx, k.m, k.S, k.h, x, y, k.thr); }
};

// The count pass of plane `inst` by the 16 waves of its block (RLE_SEGS x 64 threads): per segment its transitions and the position of the
// last one; per plane its runs, area and tight box (areas / bboxes may be null).
template <class Bit>
__device__ __forceinline__ void rle_count_plane(const RleWalk& k, Bit bit, size_t inst, RleSeg* __restrict__ segs, uint32_t* __restrict__ nruns,
                                                uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t count = 0, last = 0, area = 0;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (long it = k.items * wave / RLE_SEGS, end = k.items * (wave + 1) / RLE_SEGS; it < end; ++it) {
        const RleChunk c = rle_chunk_of(k, it, lane, bit);
        if (c.trans) { count += __popcll(c.trans); last = c.p0 + (63 - __clzll(c.trans)); }
        if (c.set) {
            area += __popcll(c.set);
            xmin = min(xmin, c.x); xmax = max(xmax, c.x);
            ymin = min(ymin, c.y0 + (__ffsll(c.set) - 1)); ymax = max(ymax, c.y0 + 63 - __clzll(c.set));
        }
    }
    __shared__ uint32_t s_count[RLE_SEGS], s_area[RLE_SEGS];
    __shared__ int s_box[RLE_SEGS][4];
    if (lane == 0) {
        segs[inst * RLE_SEGS + wave] = RleSeg{count, last};
        s_count[wave] = count; s_area[wave] = area;
        s_box[wave][0] = xmin; s_box[wave][1] = ymin; s_box[wave][2] = xmax; s_box[wave][3] = ymax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int s = 1; s < RLE_SEGS; ++s) {
            count += s_count[s]; area += s_area[s];
            xmin = min(xmin, s_box[s][0]); ymin = min(ymin, s_box[s][1]); xmax = max(xmax, s_box[s][2]); ymax = max(ymax, s_box[s][3]);
        }
        nruns[inst] = count + 1;
        if (areas) areas[inst] = area;
        if (bboxes) {
            int* o = bboxes + inst * 4;
            const bool any = area > 0;
            o[0] = any ? xmin : 0; o[1] = any ? ymin : 0; o[2] = any ? xmax - xmin + 1 : 0; o[3] = any ? ymax - ymin + 1 : 0;
        }
    }
}

// The write pass: the same walk; a wave starts at the plane's offset + the transitions of the segments before its own, with the last
// transition before its segment as predecessor, and stores p_k - p_(k-1) per transition; the last wave adds h*w - p_T.  Nothing is stored
// at or behind `stop`.
template <class Bit>
__device__ __forceinline__ void rle_write_plane(const RleWalk& k, Bit bit, size_t inst, const RleSeg* __restrict__ segs, long long off, long long stop,
                                                uint32_t* __restrict__ counts)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t prev = 0;                                                     // the transition before this wave's first; 0 = the plane's start
    for (int s = 0; s < wave; ++s) {
        const RleSeg g = segs[inst * RLE_SEGS + s];
        if (g.count) { off += g.count; prev = g.last; }
    }
    for (long it = k.items * wave / RLE_SEGS, end = k.items * (wave + 1) / RLE_SEGS; it < end; ++it) {
        const RleChunk c = rle_chunk_of(k, it, lane, bit);
        if (!c.trans) continue;
        if ((c.trans >> lane) & 1ull) {
            const unsigned long long below = c.trans & ((1ull << lane) - 1ull);
            const long long at = off + __popcll(below);
            // the transition before mine: the nearest one below me in this chunk (lanes are consecutive positions), else `prev`
            const uint32_t run = below ? (uint32_t)(lane - (63 - __clzll(below))) : c.p0 + (uint32_t)lane - prev;
            if (at < stop) counts[at] = run;
        }
        off += __popcll(c.trans);
        prev = c.p0 + (63 - __clzll(c.trans));
    }
    if (wave == RLE_SEGS - 1 && lane == 0 && off < stop) counts[off] = (uint32_t)k.h * (uint32_t)k.w - prev;
}

}  // namespace mrcnn
