// kernels_tiles.hip — mrcnn_merge_tiles on gfx950 (wave64): the records of overlapping windows in the frame of the image they were cut
// from, the duplicates of the overlaps dropped.  tiles_host.cpp is the definition; every decision here has its bits.
//
// A fixed number of launches whatever the number of tiles:
//   k_unletterbox_boxes  (kernels_roialign.hip, launched by the caller) the pixel box of every candidate in its tile
//   k_tiles_shift        the box moved by the tile's origin into the full frame, and the source-frame row (double quotients)
//   k_rle_count / k_rle_offsets / k_rle_write   (kernels_roialign.hip, unchanged) the candidates' planes as COCO RLE in the full frame:
//                        paste_tap only sees `pixel - box origin`, so a shifted box under a table entry carrying the IMAGE's h and w
//                        encodes the tile's plane embedded in the image
//   k_tiles_sort         one workgroup per image: its candidates sorted by (score descending, k ascending) in LDS (bitonic on unique
//                        48-bit keys — deterministic, hence the stable order); 8192 keys x 6 B = 48 KiB of LDS, one block per CU
//   k_tiles_pairs        one wave per (candidate c, 64 earlier places): lanes pre-test (class, tile, boxes) and only the survivors
//                        walk the two run lists for the exact intersection; the verdicts leave as ONE 64-bit ballot word per wave
//                        (a plain vector store, no atomics)
//   k_tiles_scan         one wave per image: the greedy walk over the bit rows, kept set in registers (2 words per lane); the rows
//                        of the next places are requested before the current one is resolved (they do not depend on the verdicts)
//   k_tiles_out_count / k_rle_offsets / k_tiles_out_write   the kept candidates' runs, areas and boxes compacted into the output
// mrcnn_unite_tiles shares the first four and has its own selection (further down): links, components, union planes.
// Compiled with -ffp-contract=off: the quotients are IEEE double divisions of exact integers.
#include "kernels_tiles.h"
#include "rle_device.h"

namespace mrcnn {

// defined in kernels_roialign.hip
__global__ void k_rle_count(const ImageGeom* __restrict__ tab, const int4* __restrict__ boxes, const float* __restrict__ masks, int rows, int S,
                            float thr, RleSeg* __restrict__ segs, uint32_t* __restrict__ nruns, uint32_t* __restrict__ areas,
                            int32_t* __restrict__ bboxes);
__global__ void k_rle_offsets(const uint32_t* __restrict__ nruns, int total, long long* __restrict__ run_offsets);

constexpr int TILES_LIMIT = MRCNN_TILES_MAX_CANDIDATES;        // candidates per image the LDS sort holds
static_assert(TILES_LIMIT == 8192 && TILES_LIMIT / 64 == 128, "k_tiles_scan keeps two 64-bit words per lane");

__global__ __launch_bounds__(256) void k_tiles_shift(const TileGeom* __restrict__ tiles, const float* __restrict__ det, int rows, int total,
                                                     int4* __restrict__ boxes, float* __restrict__ rows_src)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const TileGeom t = tiles[i / rows];
    int4 b = boxes[i];
    float r[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b.z > b.x) {                                           // (not eligible = (0,0,0,0), as k_unletterbox_boxes leaves it)
        b.x += t.y0; b.y += t.x0; b.z += t.y0; b.w += t.x0;
        const double hy = t.img_h > 1 ? t.img_h - 1 : 1, wx = t.img_w > 1 ? t.img_w - 1 : 1;
        r[0] = (float)((double)b.x / hy); r[1] = (float)((double)b.y / wx);
        r[2] = (float)((double)(b.z - 1) / hy); r[3] = (float)((double)(b.w - 1) / wx);
        r[4] = det[(size_t)i * 6 + 4]; r[5] = det[(size_t)i * 6 + 5];
        boxes[i] = b;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) rows_src[(size_t)i * 6 + k] = r[k];
}

// candidate s of image b's list: its tiles in ascending order, each with `rows` rows — ascending in k
__device__ __forceinline__ int tiles_candidate(const int* __restrict__ tlist, int t0, int rows, int s) { return tlist[t0 + s / rows] * rows + s % rows; }

__global__ __launch_bounds__(1024) void k_tiles_sort(const int* __restrict__ toff, const int* __restrict__ tlist, int rows,
                                                     const float* __restrict__ det, const int4* __restrict__ boxes, int* __restrict__ order,
                                                     int* __restrict__ pos, int* __restrict__ nelig)
{
    __shared__ uint32_t s_key[TILES_LIMIT];                    // the score's bits (> 0 for an eligible candidate: its score is > 0), 0 = not eligible
    __shared__ uint16_t s_idx[TILES_LIMIT];                    // its place in the image's list
    __shared__ int s_n;
    const int b = blockIdx.x, t = threadIdx.x, t0 = toff[b];
    const int n = (toff[b + 1] - t0) * rows;                   // <= TILES_LIMIT (checked on the host)
    int P = 64;
    while (P < n) P <<= 1;
    if (t == 0) s_n = 0;
    for (int s = t; s < P; s += 1024) {
        uint32_t key = 0;
        if (s < n) {
            const int k = tiles_candidate(tlist, t0, rows, s);
            const int4 bx = boxes[k];
            if (bx.z > bx.x) key = __float_as_uint(det[(size_t)k * 6 + 5]);
        }
        s_key[s] = key; s_idx[s] = (uint16_t)(s < n ? s : 0xffff);
    }
    __syncthreads();
    auto comp = [&](int i) { return ((unsigned long long)(~s_key[i]) << 16) | s_idx[i]; };     // ascending = score descending, then k ascending
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 1024) {
                const int x = i ^ j;
                if (x > i) {
                    const bool up = (i & k2) == 0;
                    if ((comp(i) > comp(x)) == up) {
                        const uint32_t ka = s_key[i]; s_key[i] = s_key[x]; s_key[x] = ka;
                        const uint16_t ia = s_idx[i]; s_idx[i] = s_idx[x]; s_idx[x] = ia;
                    }
                }
            }
            __syncthreads();
        }
    for (int r = t; r < P; r += 1024)                          // the eligible ones come first: the last of them names their number
        if (s_key[r] != 0 && (r == P - 1 || s_key[r + 1] == 0)) s_n = r + 1;
    __syncthreads();
    const int ne = s_n;
    for (int r = t; r < P; r += 1024) {
        const int s = s_idx[r];
        if (s == 0xffff) continue;                             // (padding of the power of two)
        const int k = tiles_candidate(tlist, t0, rows, s);
        if (r < ne) order[t0 * rows + r] = k;
        pos[k] = r < ne ? r : -1;
    }
    if (t == 0) nelig[b] = ne;
}

// |A ∧ B| of two COCO run lists over the same plane (tiles_host.cpp: intersection)
__device__ __forceinline__ uint32_t tiles_intersection(const uint32_t* __restrict__ a, int na, const uint32_t* __restrict__ b, int nb)
{
    uint32_t inter = 0, at = 0, pa = a[0], pb = b[0];          // (every list has at least one run; a plane has < 2^30 pixels)
    int ia = 0, ib = 0;
    while (ia < na && ib < nb) {
        const uint32_t to = pa < pb ? pa : pb;
        if ((ia & 1) && (ib & 1)) inter += to - at;
        at = to;
        if (pa == to) { ++ia; if (ia < na) pa += a[ia]; }
        if (pb == to) { ++ib; if (ib < nb) pb += b[ib]; }
    }
    return inter;
}

__global__ __launch_bounds__(256) void k_tiles_pairs(const TileGeom* __restrict__ tiles, const int* __restrict__ toff, int rows, int total,
                                                     const float* __restrict__ det, const int4* __restrict__ boxes,
                                                     const uint32_t* __restrict__ counts, const long long* __restrict__ ro,
                                                     const uint32_t* __restrict__ areas, const int* __restrict__ order, const int* __restrict__ pos,
                                                     int metric, double match_thr, int W, unsigned long long* __restrict__ supp)
{
    const int c = blockIdx.x, lane = threadIdx.x & 63;         // (x: the candidates may be more than a grid's y extent)
    const int word = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int rc = pos[c];
    if (rc < 0 || word >= W || word * 64 > rc) return;          // (wave-uniform; k_tiles_scan reads words 0 .. rc / 64 of row c only)
    const int base = toff[tiles[c / rows].image] * rows;
    const int rq = word * 64 + lane;
    bool hit = false;
    if (rq < rc) {
        const int q = order[base + rq];
        const int4 bc = boxes[c], bq = boxes[q];
        const bool pre = q / rows != c / rows && det[(size_t)q * 6 + 4] == det[(size_t)c * 6 + 4] &&
                         max(bc.x, bq.x) < min(bc.z, bq.z) && max(bc.y, bq.y) < min(bc.w, bq.w);
        if (pre) {
            const uint32_t inter = tiles_intersection(counts + ro[q], (int)(ro[q + 1] - ro[q]), counts + ro[c], (int)(ro[c + 1] - ro[c]));
            const unsigned long long aq = areas[q], ac = areas[c];
            const unsigned long long den = metric == MRCNN_MATCH_IOU ? aq + ac - inter : (aq < ac ? aq : ac);
            const double m = den == 0 ? 0.0 : (double)inter / (double)den;
            hit = m >= match_thr;
        }
    }
    const unsigned long long bits = __ballot(hit);
    if (lane == 0) supp[(size_t)c * W + word] = bits;
}

__global__ __launch_bounds__(64) void k_tiles_scan(const int* __restrict__ toff, int rows, const int* __restrict__ order, const int* __restrict__ nelig,
                                                   const unsigned long long* __restrict__ supp, int W, const float* __restrict__ rows_src, int max_out,
                                                   float* __restrict__ det_src, int32_t* __restrict__ source, int32_t* __restrict__ n_kept)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int base = toff[b] * rows, n = nelig[b];
    unsigned long long kept0 = 0, kept1 = 0;                   // lane l: words l and l + 64 of the kept set (W <= 128)
    int kc = 0;
    constexpr int U = 8;
    for (int r0 = 0; r0 < n; r0 += U) {
        int cand[U];
        unsigned long long w0[U], w1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                          // the bit rows of the next U places: independent of what gets kept
            const int r = r0 + u;
            cand[u] = r < n ? order[base + r] : -1;
            const int nw = r / 64 + 1;
            w0[u] = (r < n && lane < nw) ? supp[(size_t)cand[u] * W + lane] : 0ull;
            w1[u] = (r < n && lane + 64 < nw) ? supp[(size_t)cand[u] * W + lane + 64] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = r0 + u;
            if (r >= n) break;
            if (__ballot(((w0[u] & kept0) | (w1[u] & kept1)) != 0ull) != 0ull) continue;       // dropped: it suppresses nothing
            const int wd = r >> 6;
            if (lane == (wd & 63)) { if (wd < 64) kept0 |= 1ull << (r & 63); else kept1 |= 1ull << (r & 63); }
            if (kc < max_out) {
                const size_t slot = (size_t)b * max_out + kc;
                if (lane < 6) det_src[slot * 6 + lane] = rows_src[(size_t)cand[u] * 6 + lane];
                if (lane == 6) source[slot] = cand[u];
            }
            ++kc;
        }
    }
    if (lane == 0) n_kept[b] = kc;
    for (int j = kc + lane; j < max_out; j += 64) {
        const size_t slot = (size_t)b * max_out + j;
        source[slot] = -1;
#pragma unroll
        for (int k = 0; k < 6; ++k) det_src[slot * 6 + k] = 0.f;
    }
}

__global__ __launch_bounds__(256) void k_tiles_out_count(const int32_t* __restrict__ source, int slots, const uint32_t* __restrict__ nruns,
                                                         const uint32_t* __restrict__ areas, const int32_t* __restrict__ bboxes,
                                                         uint32_t* __restrict__ out_nruns, uint32_t* __restrict__ out_areas,
                                                         int32_t* __restrict__ out_bboxes)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const int k = source[s];
    out_nruns[s] = k >= 0 ? nruns[k] : 1u;                     // padding: the single run [h*w]
    if (out_areas) out_areas[s] = k >= 0 ? areas[k] : 0u;
    if (out_bboxes) {
#pragma unroll
        for (int j = 0; j < 4; ++j) out_bboxes[(size_t)s * 4 + j] = k >= 0 ? bboxes[(size_t)k * 4 + j] : 0;
    }
}

__global__ __launch_bounds__(256) void k_tiles_out_write(const int32_t* __restrict__ source, int max_out, const int2* __restrict__ imgsz,
                                                         const uint32_t* __restrict__ counts, const long long* __restrict__ ro,
                                                         const long long* __restrict__ out_ro, uint32_t* __restrict__ out_counts)
{
    const int s = blockIdx.x, k = source[s];
    const long long o0 = out_ro[s], o1 = out_ro[s + 1];
    if (k < 0) {
        const int2 sz = imgsz[s / max_out];
        if (threadIdx.x == 0 && o0 < o1) out_counts[o0] = (uint32_t)sz.x * (uint32_t)sz.y;
        return;
    }
    const uint32_t* src = counts + ro[k];
    for (long long i = threadIdx.x; i < o1 - o0; i += 256) out_counts[o0 + i] = src[i];
}

void tiles_rle_count_forward(hipStream_t s, const TilesMerge& m)
{
    const int total = m.n_tiles * m.rows;
    hipLaunchKernelGGL(k_tiles_shift, dim3((total + 255) / 256), dim3(256), 0, s, m.tiles, m.det, m.rows, total, m.boxes, m.rows_src);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_rle_count, dim3(total), dim3(64 * RLE_SEGS), 0, s, m.tab_full, (const int4*)m.boxes, m.masks, m.rows, m.S, m.thr, m.segs,
                       m.nruns, m.areas, m.bboxes);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(1024), 0, s, (const uint32_t*)m.nruns, total, m.ro);
    HIP_CHECK(hipGetLastError());
}

void tiles_order_forward(hipStream_t s, const TilesMerge& m)
{
    MRCNN_REQUIRE(m.W >= 1 && m.W <= TILES_LIMIT / 64, MRCNN_ERR_SHAPE, "merge_tiles: %d suppression words per row", m.W);
    masks_rle_write_forward(s, m.masks, m.tab_full, m.n_tiles, m.rows, m.S, m.thr, m.boxes, m.segs, m.ro, m.counts);
    hipLaunchKernelGGL(k_tiles_sort, dim3(m.n_images), dim3(1024), 0, s, m.toff, m.tlist, m.rows, m.det, (const int4*)m.boxes, m.order, m.pos, m.nelig);
    HIP_CHECK(hipGetLastError());
}

void tiles_select_forward(hipStream_t s, const TilesMerge& m)
{
    const int total = m.n_tiles * m.rows, slots = m.n_images * m.max_out;
    hipLaunchKernelGGL(k_tiles_pairs, dim3(total, (m.W + 3) / 4), dim3(256), 0, s, m.tiles, m.toff, m.rows, total, m.det, (const int4*)m.boxes,
                       (const uint32_t*)m.counts, (const long long*)m.ro, (const uint32_t*)m.areas, (const int*)m.order, (const int*)m.pos, m.metric,
                       m.match_thr, m.W, m.supp);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tiles_scan, dim3(m.n_images), dim3(64), 0, s, m.toff, m.rows, (const int*)m.order, (const int*)m.nelig,
                       (const unsigned long long*)m.supp, m.W, (const float*)m.rows_src, m.max_out, m.det_src, m.source, m.n_kept);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tiles_out_count, dim3((slots + 255) / 256), dim3(256), 0, s, (const int32_t*)m.source, slots, (const uint32_t*)m.nruns,
                       (const uint32_t*)m.areas, (const int32_t*)m.bboxes, m.out_nruns, m.out_areas, m.out_bboxes);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(1024), 0, s, (const uint32_t*)m.out_nruns, slots, m.out_ro);
    HIP_CHECK(hipGetLastError());
}

void tiles_gather_forward(hipStream_t s, const TilesMerge& m)
{
    const int slots = m.n_images * m.max_out;
    hipLaunchKernelGGL(k_tiles_out_write, dim3(slots), dim3(256), 0, s, (const int32_t*)m.source, m.max_out, m.imgsz, (const uint32_t*)m.counts,
                       (const long long*)m.ro, (const long long*)m.out_ro, m.out_counts);
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// mrcnn_unite_tiles: the cut parts of an object united into one mask.  The staging above (boxes, runs, order) is the merge's; then
//   k_unite_links    k_tiles_pairs' layout; the verdict is the agreement of the two planes inside the rectangle R both windows see:
//                    one walk over the two run lists yields |Pq ∧ Pc|, |Pq ∧ R| and |Pc ∧ R| (tiles_inside at the segment ends)
//   k_unite_comp     one workgroup per image: the connected components of the link bits by min-label propagation in LDS (atomicMin on
//                    both ends of a link, pointer jumping, until nothing changes: the fixed point — every label the least place of its
//                    component — is unique, so the order in which the atomics land does not show), a sort of (label, place) keys that
//                    groups the members by component in place order, and a scan over the group heads
//   k_unite_count / k_rle_offsets / k_unite_write   per output slot the walk of rle_device.h over the hull of the members' boxes, the
//                    bit the OR of the members' paste bits: no plane is written, and every bit is paste_pixel's
// ------------------------------------------------------------------------------------------------

// the positions p < n of a plane of height h that lie inside r = (y0, x0, y1, x1), far edges exclusive (tiles_host.cpp: inside)
__device__ __forceinline__ int tiles_inside(const int4 r, uint32_t h, uint32_t n)
{
    const int x = (int)(n / h), y = (int)(n - (uint32_t)x * h), rw = r.w - r.y, rh = r.z - r.x;
    const int full = min(max(x - r.y, 0), rw);
    const int part = (x >= r.y && x < r.w) ? min(max(y - r.x, 0), rh) : 0;
    return full * rh + part;                                   // (<= the plane: < 2^30)
}

__global__ __launch_bounds__(256) void k_unite_links(const TileGeom* __restrict__ tiles, const int* __restrict__ toff, int rows, int total,
                                                     const float* __restrict__ det, const int4* __restrict__ boxes,
                                                     const uint32_t* __restrict__ counts, const long long* __restrict__ ro,
                                                     const int* __restrict__ order, const int* __restrict__ pos, int metric, double link_thr, int W,
                                                     unsigned long long* __restrict__ link)
{
    const int c = blockIdx.x, lane = threadIdx.x & 63;
    const int word = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int rc = pos[c];
    if (rc < 0 || word >= W || word * 64 > rc) return;          // (wave-uniform; k_unite_comp reads words 0 .. rc / 64 of row c only)
    const TileGeom tc = tiles[c / rows];
    const int base = toff[tc.image] * rows;
    const int rq = word * 64 + lane;
    bool hit = false;
    if (rq < rc) {
        const int q = order[base + rq];
        const TileGeom tq = tiles[q / rows];
        const int4 bc = boxes[c], bq = boxes[q];
        const int4 r = make_int4(max(tq.y0, tc.y0), max(tq.x0, tc.x0), min(tq.y0 + tq.th, tc.y0 + tc.th), min(tq.x0 + tq.tw, tc.x0 + tc.tw));
        // (boxes that do not meet have an empty intersection: the measure is 0 and the threshold is > 0)
        const bool pre = q / rows != c / rows && det[(size_t)q * 6 + 4] == det[(size_t)c * 6 + 4] && r.x < r.z && r.y < r.w &&
                         max(bc.x, bq.x) < min(bc.z, bq.z) && max(bc.y, bq.y) < min(bc.w, bq.w);
        if (pre) {
            const uint32_t *a = counts + ro[q], *b = counts + ro[c];
            const int na = (int)(ro[q + 1] - ro[q]), nb = (int)(ro[c + 1] - ro[c]);
            const uint32_t h = (uint32_t)tc.img_h;
            uint32_t inter = 0, aq = 0, ac = 0, at = 0, pa = a[0], pb = b[0];       // (both lists end at h*w: one loop serves)
            int ia = 0, ib = 0, fat = 0;
            while (ia < na && ib < nb) {
                const uint32_t to = pa < pb ? pa : pb;
                const int fto = tiles_inside(r, h, to);
                if (ia & 1) aq += (uint32_t)(fto - fat);
                if (ib & 1) ac += (uint32_t)(fto - fat);
                if (ia & ib & 1) inter += to - at;
                at = to; fat = fto;
                if (pa == to) { ++ia; if (ia < na) pa += a[ia]; }
                if (pb == to) { ++ib; if (ib < nb) pb += b[ib]; }
            }
            const unsigned long long den = metric == MRCNN_MATCH_IOU ? (unsigned long long)aq + ac - inter : (aq < ac ? aq : ac);
            const double m = den == 0 ? 0.0 : (double)inter / (double)den;
            hit = m >= link_thr;
        }
    }
    const unsigned long long bits = __ballot(hit);
    if (lane == 0) link[(size_t)c * W + word] = bits;
}

constexpr int TILES_PLACE_BITS = 13;
static_assert(TILES_LIMIT == 1 << TILES_PLACE_BITS && TILES_LIMIT == 8 * 1024, "k_unite_comp: 8 places per thread, (label, place) in 26 bits");

__global__ __launch_bounds__(1024) void k_unite_comp(const int* __restrict__ toff, const int* __restrict__ tlist, int rows,
                                                     const int* __restrict__ order, const int* __restrict__ pos, const int* __restrict__ nelig,
                                                     const unsigned long long* __restrict__ link, int W, int max_out, int32_t* __restrict__ source,
                                                     int32_t* __restrict__ n_kept, int32_t* __restrict__ group, int* __restrict__ members,
                                                     int2* __restrict__ mspan)
{
    __shared__ unsigned int s_lab[TILES_LIMIT];                // the label of place r; later the sorted keys (label << 13 | place)
    __shared__ int s_scan[2][1024];
    __shared__ int s_changed;
    const int b = blockIdx.x, t = threadIdx.x, t0 = toff[b];
    const int base = t0 * rows, n = nelig[b], nall = (toff[b + 1] - t0) * rows;
    for (int r = t; r < n; r += 1024) s_lab[r] = (unsigned)r;
    if (t == 0) s_changed = 0;
    __syncthreads();
    for (;;) {
        for (int r = t; r < n; r += 1024) {                    // every link (q, r), q < r: the smaller label to the other end
            const unsigned long long* row = link + (size_t)order[base + r] * W;
            for (int w = 0; w <= (r >> 6); ++w) {
                unsigned long long bits = row[w];
                while (bits) {
                    const int q = w * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const unsigned lq = s_lab[q], lr = s_lab[r];
                    if (lq < lr) { atomicMin(&s_lab[r], lq); s_changed = 1; }
                    else if (lr < lq) { atomicMin(&s_lab[q], lr); s_changed = 1; }
                }
            }
        }
        __syncthreads();
        for (int r = t; r < n; r += 1024) {                    // pointer jumping: a label is a place of the same component
            const unsigned l = s_lab[r], ll = s_lab[l];
            if (ll < l) { atomicMin(&s_lab[r], ll); s_changed = 1; }
        }
        __syncthreads();
        const int changed = s_changed;
        __syncthreads();
        if (!changed) break;                                   // (a round that wrote nothing read only settled labels)
        if (t == 0) s_changed = 0;
        __syncthreads();
    }
    // the members grouped by component (= by label: components are listed by their representative's place), in place order
    int P = 64;
    while (P < n) P <<= 1;
    for (int r = t; r < TILES_LIMIT; r += 1024) s_lab[r] = r < n ? (s_lab[r] << TILES_PLACE_BITS) | (unsigned)r : 0xffffffffu;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 1024) {
                const int x = i ^ j;
                if (x > i) {
                    const bool up = (i & k2) == 0;
                    const unsigned a = s_lab[i], c = s_lab[x];
                    if ((a > c) == up) { s_lab[i] = c; s_lab[x] = a; }
                }
            }
            __syncthreads();
        }
    // thread t owns the sorted places 8t .. 8t + 7: the heads among them, scanned over the block
    auto head = [&](int j) { return j < n && (j == 0 || (s_lab[j - 1] >> TILES_PLACE_BITS) != (s_lab[j] >> TILES_PLACE_BITS)); };
    int mine = 0;
    for (int j = t * 8; j < t * 8 + 8; ++j) mine += head(j) ? 1 : 0;
    int cur = 0;
    s_scan[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int ncomp = s_scan[cur][1023];
    int ci = s_scan[cur][t] - mine - 1;                        // the component of the place before mine
    for (int j = t * 8; j < t * 8 + 8 && j < n; ++j) {
        const bool hd = head(j);
        if (hd) ++ci;
        const int k = order[base + (int)(s_lab[j] & (TILES_LIMIT - 1))];
        group[k] = ci;
        members[base + j] = k;
        if (ci < max_out) {
            const size_t slot = (size_t)b * max_out + ci;
            if (hd) { source[slot] = k; mspan[slot].x = base + j; }          // (the head is the least place: the representative)
            if (j == n - 1 || head(j + 1)) mspan[slot].y = base + j + 1;
        }
    }
    if (t == 0) n_kept[b] = ncomp;
    for (int j = ncomp + t; j < max_out; j += 1024) {
        const size_t slot = (size_t)b * max_out + j;
        source[slot] = -1; mspan[slot] = make_int2(0, 0);
    }
    for (int s = t; s < nall; s += 1024) {
        const int k = tiles_candidate(tlist, t0, rows, s);
        if (pos[k] < 0) group[k] = -1;
    }
}

// the bit of the union plane: the OR of the members' paste bits
struct UniteBit {
    const int* members; int2 span; const int4* boxes; const float* masks; int S, h; float thr;
    __device__ __forceinline__ bool operator()(int x, int y) const
    {
        for (int i = span.x; i < span.y; ++i) {
            const int k = members[i];
            if (rle_bit(boxes[k], masks + (size_t)k * S * S, S, h, x, y, thr)) return true;
        }
        return false;
    }
};

__global__ __launch_bounds__(1024) void k_unite_count(const int32_t* __restrict__ source, int max_out, const int2* __restrict__ imgsz,
                                                      const int* __restrict__ members, const int2* __restrict__ mspan,
                                                      const int4* __restrict__ boxes, const float* __restrict__ masks, int S, float thr,
                                                      const float* __restrict__ rows_src, int4* __restrict__ hulls, RleSeg* __restrict__ segs,
                                                      uint32_t* __restrict__ nruns, uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes,
                                                      float* __restrict__ det_src, int32_t* __restrict__ n_parts)
{
    const int slot = blockIdx.x;
    const int src = source[slot];
    if (src < 0) {                                             // padding: the single run [h*w] (block-uniform)
        if (threadIdx.x == 0) {
            nruns[slot] = 1u; areas[slot] = 0u; n_parts[slot] = 0; hulls[slot] = make_int4(0, 0, 0, 0);
            for (int j = 0; j < 4; ++j) bboxes[(size_t)slot * 4 + j] = 0;
            for (int j = 0; j < 6; ++j) det_src[(size_t)slot * 6 + j] = 0.f;
        }
        return;
    }
    const int2 span = mspan[slot], sz = imgsz[slot / max_out];
    __shared__ int s_hull[4];
    if (threadIdx.x == 0) { s_hull[0] = s_hull[1] = 0x7fffffff; s_hull[2] = s_hull[3] = -1; }
    __syncthreads();
    for (int i = span.x + (int)threadIdx.x; i < span.y; i += 1024) {
        const int4 bx = boxes[members[i]];
        atomicMin(&s_hull[0], bx.x); atomicMin(&s_hull[1], bx.y); atomicMax(&s_hull[2], bx.z); atomicMax(&s_hull[3], bx.w);
    }
    __syncthreads();
    RleWalk k;
    k.bx = make_int4(s_hull[0], s_hull[1], s_hull[2], s_hull[3]); k.m = nullptr; k.S = S; k.h = sz.x; k.w = sz.y; k.thr = thr;
    rle_walk_box(k);
    if (threadIdx.x == 0) {                                    // the row of the hull, as k_tiles_shift writes a candidate's
        const double hy = sz.x > 1 ? sz.x - 1 : 1, wx = sz.y > 1 ? sz.y - 1 : 1;
        float* o = det_src + (size_t)slot * 6;
        o[0] = (float)((double)k.bx.x / hy); o[1] = (float)((double)k.bx.y / wx);
        o[2] = (float)((double)(k.bx.z - 1) / hy); o[3] = (float)((double)(k.bx.w - 1) / wx);
        o[4] = rows_src[(size_t)src * 6 + 4]; o[5] = rows_src[(size_t)src * 6 + 5];
        hulls[slot] = k.bx; n_parts[slot] = span.y - span.x;
    }
    rle_count_plane(k, UniteBit{members, span, boxes, masks, S, sz.x, thr}, (size_t)slot, segs, nruns, areas, bboxes);
}

__global__ __launch_bounds__(1024) void k_unite_write(const int32_t* __restrict__ source, int max_out, const int2* __restrict__ imgsz,
                                                      const int* __restrict__ members, const int2* __restrict__ mspan,
                                                      const int4* __restrict__ boxes, const float* __restrict__ masks, int S, float thr,
                                                      const int4* __restrict__ hulls, const RleSeg* __restrict__ segs,
                                                      const long long* __restrict__ run_offsets, uint32_t* __restrict__ counts)
{
    const int slot = blockIdx.x;
    const int2 sz = imgsz[slot / max_out];
    const long long off = run_offsets[slot];
    const long long stop = run_offsets[slot + 1];              // nothing of this slot is stored at or behind it
    if (source[slot] < 0) {
        if (threadIdx.x == 0 && off < stop) counts[off] = (uint32_t)sz.x * (uint32_t)sz.y;
        return;
    }
    RleWalk k;
    k.bx = hulls[slot]; k.m = nullptr; k.S = S; k.h = sz.x; k.w = sz.y; k.thr = thr;
    rle_walk_box(k);
    rle_write_plane(k, UniteBit{members, mspan[slot], boxes, masks, S, sz.x, thr}, (size_t)slot, segs, off, stop, counts);
}

void tiles_unite_forward(hipStream_t s, const TilesMerge& m)
{
    const int total = m.n_tiles * m.rows, slots = m.n_images * m.max_out;
    hipLaunchKernelGGL(k_unite_links, dim3(total, (m.W + 3) / 4), dim3(256), 0, s, m.tiles, m.toff, m.rows, total, m.det, (const int4*)m.boxes,
                       (const uint32_t*)m.counts, (const long long*)m.ro, (const int*)m.order, (const int*)m.pos, m.metric, m.match_thr, m.W, m.supp);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_unite_comp, dim3(m.n_images), dim3(1024), 0, s, m.toff, m.tlist, m.rows, (const int*)m.order, (const int*)m.pos,
                       (const int*)m.nelig, (const unsigned long long*)m.supp, m.W, m.max_out, m.source, m.n_kept, m.group, m.members, m.mspan);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_unite_count, dim3(slots), dim3(64 * RLE_SEGS), 0, s, (const int32_t*)m.source, m.max_out, m.imgsz, (const int*)m.members,
                       (const int2*)m.mspan, (const int4*)m.boxes, m.masks, m.S, m.thr, (const float*)m.rows_src, m.hull, m.out_segs, m.out_nruns,
                       m.out_areas, m.out_bboxes, m.det_src, m.n_parts);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(1024), 0, s, (const uint32_t*)m.out_nruns, slots, m.out_ro);
    HIP_CHECK(hipGetLastError());
}

void tiles_unite_write_forward(hipStream_t s, const TilesMerge& m)
{
    const int slots = m.n_images * m.max_out;
    hipLaunchKernelGGL(k_unite_write, dim3(slots), dim3(64 * RLE_SEGS), 0, s, (const int32_t*)m.source, m.max_out, m.imgsz, (const int*)m.members,
                       (const int2*)m.mspan, (const int4*)m.boxes, m.masks, m.S, m.thr, (const int4*)m.hull, (const RleSeg*)m.out_segs,
                       (const long long*)m.out_ro, m.out_counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
