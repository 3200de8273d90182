// kernels_rle_draw.hip — drawing run-length masks on gfx950: the dense planes, the instance-id map and the rendered overlay of a ragged
// batch of mixed-size images from an RLE set (mrcnn_rle_decode, mrcnn_instance_map_rle, mrcnn_render_detections_rle).  What
// kernels_render.hip does for 28×28 masks, for masks that exist only as runs: the output of mrcnn_merge_tiles / mrcnn_unite_tiles,
// of mrcnn_masks_rle_source and of the ground-truth encoder.  rle_draw_host.cpp is the definition; the kernels give its bytes.
//
// The runs are column-major (position p = x*h + y), every output is row-major, so a block goes through LDS.
//
//   pass 1  rle_prefix_forward (kernels_rle_prefix.hip): per RLE the table B (B[j] = the position where run j starts), its total and the
//           positions of its first and last set pixel (first / h .. last / h is its exact column extent: the cull key);
//           k_rle_draw_prepare: one record per RLE (runs, extent, pixel box, drawn) and ONE word for the check of the totals against h*w.
//   pass 2  k_rle_draw<MODE>: one launch for the whole ragged batch, grid (tiles, images) — (tiles, planes) for the decode.
//
// A block owns a tile of TH = 32 rows × TW = 256 columns of one image and keeps the tile's owners in LDS: int16 ids for the map
// (16 KiB), one code byte per pixel for the overlay and the plane (8 KiB).  TW = 256 gives every thread of the block one column, so a
// column of the tile has ONE writer: claiming a pixel needs no LDS atomic, and the list is walked in ascending row index, so the
// first claim is the lowest row's and final.  A row of the tile goes out as 256 (plane), 512 (map) or 768 (overlay) consecutive bytes.
// TH = 32 amortises one binary search in B over up to 32 positions (a flat row-major tile pays one per pixel); twice the height
// would halve the searches again but a 4096 × 3072 image has only 1536 tiles as it is, six per CU.  With the list and the counters a block
// holds 8 KiB (plane), 19 KiB (overlay) or 31 KiB (map) of the CU's 160 KiB LDS: five blocks per CU for the map, more for the others.
//
// Per tile the block culls the image's drawn RLEs to those whose column extent meets the tile's columns (the overlay: or whose
// stroke meets the tile) into an LDS list in ascending row index, 256 per pass, ballot + popcount for the position, as
// kernels_render.hip does; more than 256 slots take further passes over the same tile.  For each listed RLE a thread finds the run
// holding (x*h + ty0) by one binary search in B and walks the runs down to (x*h + ty1), claiming the positions of ones-runs that have
// no owner.  The overlay keeps a code per pixel instead of an id: fill (lowest row) and ring (lowest row, over any fill), the ring
// evaluated from the boxes.  visible_areas: a thread counts its claims per listed row, adds them to an LDS counter, then one global
// atomic per (block, row) that has any.
//
// B is read from global memory (L2), never staged in LDS — a different form from a staged table, for this reason: the runs a tile needs
// of one RLE are the few around 256 column segments, found by search, so staging them means a search per RLE by the block first and a
// barrier per listed RLE, where now every thread goes through the whole list on its own; and an RLE with more runs than a staging
// holds would need this path anyway.  A walk reads consecutive B entries, and neighbouring columns read neighbouring ones.
//
// Rows go out as aligned dwords where four bytes of the row fall into one, single bytes at its two ends: widths and offsets are
// arbitrary, so a row segment starts at any address; the bytes of a dword another tile also writes are never read or rewritten.
//
// Algorithmic bytes:  k_rle_draw<DECODE>   h·w written per plane
//                     k_rle_draw<MAP>      2·h·w written per image
//                     k_rle_draw<RENDER>   3·h·w read + 3·h·w written per image
// plus 4 bytes read per run a tile column crosses, and the records.
#include "kernels.h"
#include "draw_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

constexpr int RD_TH = 32, RD_TW = 256;      // the tile; RD_TW = the threads of a block
constexpr int RD_LIST = 256;                // RLEs culled per pass = the threads of a block
enum { RD_DECODE = 0, RD_MAP = 1, RD_RENDER = 2 };

struct RdList {
    RleDrawRec rec[RD_LIST];                // the listed RLEs, ascending row index
    int row[RD_LIST];
    int wave_n[RD_LIST / 64];
};

template <int MODE> struct RdTile { using type = uint8_t; };
template <> struct RdTile<RD_MAP> { using type = int16_t; };

__global__ __launch_bounds__(256) void k_rle_draw_prepare(const long long* __restrict__ run_offsets, const unsigned long long* __restrict__ totals,
                                                          const uint2* __restrict__ extent, const float* __restrict__ det, float min_score,
                                                          const ImageGeom* __restrict__ tab, long n, int slots, RleDrawRec* __restrict__ rec,
                                                          unsigned long long* __restrict__ bad)
{
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const ImageGeom im = tab[k / slots];
    if (totals[k] != (unsigned long long)im.h * (unsigned long long)im.w) atomicMin(bad, (unsigned long long)k);
    RleDrawRec r;
    r.r0 = run_offsets[k];
    r.nruns = (int)(run_offsets[k + 1] - r.r0);
    const uint2 e = extent[k];
    r.first = e.x; r.last = e.y;
    r.y1 = r.x1 = r.y2 = r.x2 = 0;
    r.drawn = 1;
    if (det) {
        const float* row = det + (size_t)k * 6;
        const RleDrawBox b = rle_draw_box(row, im.h, im.w);
        r.y1 = b.y1; r.x1 = b.x1; r.y2 = b.y2; r.x2 = b.x2;
        r.drawn = rle_draw_drawn(row, b, min_score) ? 1 : 0;
    }
    rec[k] = r;
}

// One cull pass: slots [base, base + 256) of the image against the tile (inclusive bounds).  Returns the list length.  Two barriers
// inside (one of them compact_256's); the caller puts one more behind its walk before the next pass overwrites the list.
template <int MODE>
__device__ __forceinline__ int rd_cull(RdList& L, const RleDrawRec* __restrict__ rec, int slots, int base, int h, int grow, bool stroke_on,
                                       int ty0, int ty1, int tx0, int tx1)
{
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    RleDrawRec r{};
    if (i < slots) {
        r = rec[i];
        if (r.drawn) {
            keep = r.first <= r.last && (int)(r.first / (uint32_t)h) <= tx1 && (int)(r.last / (uint32_t)h) >= tx0;
            if (MODE == RD_RENDER && stroke_on)
                keep |= r.y1 - grow <= ty1 && r.y2 + grow > ty0 && r.x1 - grow <= tx1 && r.x2 + grow > tx0;
        }
    }
    int n;
    const int pos = compact_256(keep, L.wave_n, &n);
    if (keep) {
        L.rec[pos] = r;
        L.row[pos] = i;
    }
    __syncthreads();
    return n;
}

// One RLE against one column of the tile: positions p0 .. p0 + th - 1 (column x, rows ty0 ..), col = the column's first LDS entry
// (stride RD_TW).  Returns the pixels claimed (MAP).  `total` = h*w ends the last run.
template <int MODE>
__device__ __forceinline__ uint32_t rd_walk(const RleDrawRec& r, int i, const uint32_t* __restrict__ pre_b, uint32_t total, uint32_t p0, int th,
                                            typename RdTile<MODE>::type* col)
{
    const uint32_t p1 = p0 + (uint32_t)th - 1u;
    if (r.first > r.last || r.last < p0 || r.first > p1 || r.nruns < 1) return 0;
    const uint32_t* const B = pre_b + r.r0;
    int lo = 0, hi = r.nruns - 1;                            // B[0] = 0 <= p0: the last run that starts at or before p0 holds it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (B[mid] <= p0) lo = mid; else hi = mid - 1;
    }
    uint32_t mine = 0, pos = p0;
    const uint32_t code = pixel_code(i, -1);
    for (int j = lo; pos <= p1 && j < r.nruns; ++j) {
        const uint32_t end = j + 1 < r.nruns ? B[j + 1] : total;
        const uint32_t stop = end < p1 + 1u ? end : p1 + 1u;
        if (j & 1)
            for (uint32_t q = pos; q < stop; ++q) {
                auto& c = col[(q - p0) * RD_TW];
                if constexpr (MODE == RD_DECODE) c = 1;
                else if constexpr (MODE == RD_MAP) { if (c < 0) { c = (int16_t)i; ++mine; } }
                else if (c == 0) c = (uint8_t)code;
            }
        pos = stop > pos ? stop : pos;
    }
    return mine;
}

// The tile's rows to the image: row yy of the tile is tw * UNIT consecutive bytes from (ty0 + yy, tx0).  A thread takes one aligned
// dword of one row: stored whole when all four bytes belong to the row, byte by byte at the row's two ends.
template <int MODE>
__device__ __forceinline__ void rd_emit(const typename RdTile<MODE>::type (*tile)[RD_TW], uint8_t* __restrict__ o, const uint8_t* __restrict__ src,
                                        int w, int ty0, int tx0, int th, int tw, int alpha)
{
    constexpr int UNIT = MODE == RD_DECODE ? 1 : (MODE == RD_MAP ? 2 : 3);
    constexpr int DW = RD_TW * UNIT / 4 + 1;                 // dwords a row's bytes can touch: up to 3 bytes of lead
    const int nb = tw * UNIT;
    for (int idx = threadIdx.x; idx < th * DW; idx += 256) {
        const int yy = idx / DW, d = idx - yy * DW;
        const size_t rowoff = ((size_t)(ty0 + yy) * w + tx0) * UNIT;
        uint8_t* const dst = o + rowoff;
        const int lead = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
        const int j0 = 4 * d - lead;                         // the row's byte at this dword's byte 0 (-3 .. nb + 2)
        if (j0 >= nb) continue;
        const bool whole = j0 >= 0 && j0 + 3 < nb;
        uint32_t sv = 0;
        if (MODE == RD_RENDER) {
            if (whole && ((reinterpret_cast<uintptr_t>(src + rowoff) + (uintptr_t)j0) & 3) == 0) sv = *reinterpret_cast<const uint32_t*>(src + rowoff + j0);
            else
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k >= 0 && j0 + k < nb) sv |= (uint32_t)src[rowoff + (size_t)(j0 + k)] << (8 * k);
        }
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k;
            if (j < 0 || j >= nb) continue;
            uint32_t byte;
            if constexpr (MODE == RD_DECODE) byte = tile[yy][j];
            else if constexpr (MODE == RD_MAP) byte = ((uint32_t)(uint16_t)tile[yy][j >> 1] >> (8 * (j & 1))) & 0xffu;
            else byte = render_byte((sv >> (8 * k)) & 0xffu, tile[yy][j / 3], j % 3, alpha);
            v |= byte << (8 * k);
        }
        if (whole) *reinterpret_cast<uint32_t*>(dst + j0) = v;
        else
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k >= 0 && j0 + k < nb) dst[j0 + k] = (uint8_t)(v >> (8 * k));
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rle_draw(RleDrawJob job, uint8_t* __restrict__ out, uint32_t* __restrict__ visible,
                                                  const uint8_t* const* __restrict__ srcs, int alpha, int grow, int shrink)
{
    using T = typename RdTile<MODE>::type;
    __shared__ T tile[RD_TH][RD_TW];
    const int tid = threadIdx.x;
    const long units = MODE == RD_DECODE ? (long)job.n_images * job.slots : (long)job.n_images;
    const bool stroke_on = grow + shrink > 0;
    for (long u = blockIdx.y; u < units; u += gridDim.y) {
        const int b = MODE == RD_DECODE ? (int)(u / job.slots) : (int)u;
        const ImageGeom im = job.tab[b];
        const int h = im.h, w = im.w;
        const uint32_t total = (uint32_t)h * (uint32_t)w;
        uint8_t* const o = out + im.offset + (MODE == RD_DECODE ? (size_t)(u - (long)b * job.slots) * total : (size_t)0);
        const uint8_t* const src = MODE == RD_RENDER ? srcs[b] : nullptr;
        const RleDrawRec* const rec = job.rec + (size_t)b * job.slots;
        const int tiles_x = (w + RD_TW - 1) / RD_TW, tiles_y = (h + RD_TH - 1) / RD_TH;
        for (int t = blockIdx.x; t < tiles_x * tiles_y; t += gridDim.x) {
            const int ty0 = (t / tiles_x) * RD_TH, tx0 = (t % tiles_x) * RD_TW;
            const int th = h - ty0 < RD_TH ? h - ty0 : RD_TH, tw = w - tx0 < RD_TW ? w - tx0 : RD_TW;
            const bool active = tid < tw;
            const int x = tx0 + tid;
            const uint32_t p0 = (uint32_t)x * (uint32_t)h + (uint32_t)ty0;     // (only used when active: x < w)
#pragma unroll
            for (int yy = 0; yy < RD_TH; ++yy) tile[yy][tid] = MODE == RD_MAP ? (T)-1 : (T)0;    // a column has one writer: its thread
            if constexpr (MODE == RD_DECODE) {
                if (active) rd_walk<MODE>(job.rec[u], 0, job.pre_b, total, p0, th, &tile[0][tid]);
            } else {
                __shared__ RdList L;
                __shared__ uint32_t s_cnt[RD_LIST];
                uint32_t* const vis = MODE == RD_MAP && visible ? visible + (size_t)b * job.slots : nullptr;
                for (int base = 0; base < job.slots; base += RD_LIST) {
                    s_cnt[tid] = 0;
                    const int n = rd_cull<MODE>(L, rec, job.slots, base, h, grow, stroke_on, ty0, ty0 + th - 1, tx0, tx0 + tw - 1);
                    if (active)
                        for (int e = 0; e < n; ++e) {
                            const int i = L.row[e];
                            const uint32_t mine = rd_walk<MODE>(L.rec[e], i, job.pre_b, total, p0, th, &tile[0][tid]);
                            if (MODE == RD_MAP && vis && mine) atomicAdd(&s_cnt[e], mine);
                            if constexpr (MODE == RD_RENDER) if (stroke_on) {
                                const RleDrawRec& r = L.rec[e];
                                const RleDrawBox bx{r.y1, r.x1, r.y2, r.x2};
                                if (x >= bx.x1 - grow && x < bx.x2 + grow) {
                                    const int ya = bx.y1 - grow > ty0 ? bx.y1 - grow : ty0;
                                    const int yb = bx.y2 + grow < ty0 + th ? bx.y2 + grow : ty0 + th;
                                    const T code = (T)pixel_code(-1, i);
                                    for (int y = ya; y < yb; ++y)
                                        if (!(tile[y - ty0][tid] & 0x20) && in_ring(bx, grow, shrink, y, x)) tile[y - ty0][tid] = code;
                                }
                            }
                        }
                    if (vis) {
                        __syncthreads();
                        if (tid < n && s_cnt[tid]) atomicAdd(&vis[L.row[tid]], s_cnt[tid]);
                    }
                    __syncthreads();                                    // (the next pass writes the list and the counters)
                }
            }
            __syncthreads();
            rd_emit<MODE>(tile, o, src, w, ty0, tx0, th, tw, alpha);
            __syncthreads();                                            // (the next tile clears the columns)
        }
    }
}

dim3 rd_grid(const RleDrawJob& job, long units)
{
    const long tiles = (long)((job.max_w + RD_TW - 1) / RD_TW) * ((job.max_h + RD_TH - 1) / RD_TH);
    return dim3((unsigned)(tiles < 1 ? 1 : (tiles < 4096 ? tiles : 4096)), (unsigned)(units < 65535 ? units : 65535));
}

}  // namespace

void rle_draw_prepare(hipStream_t s, const long long* run_offsets, const unsigned long long* totals, const uint2* extent, const float* det,
                      float min_score, const RleDrawJob& job, RleDrawRec* rec, unsigned long long* bad)
{
    HIP_CHECK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
    const long n = (long)job.n_images * job.slots;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rle_draw_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, run_offsets, totals, extent, det, min_score, job.tab, n,
                       job.slots, rec, bad);
    HIP_CHECK(hipGetLastError());
}

void rle_decode_forward(hipStream_t s, const RleDrawJob& job, uint8_t* out)
{
    const long units = (long)job.n_images * job.slots;
    if (units <= 0) return;
    hipLaunchKernelGGL(k_rle_draw<RD_DECODE>, rd_grid(job, units), dim3(256), 0, s, job, out, nullptr, nullptr, 0, 0, 0);
    HIP_CHECK(hipGetLastError());
}

void instance_map_rle_forward(hipStream_t s, const RleDrawJob& job, int16_t* map, uint32_t* visible)
{
    if (job.n_images <= 0) return;
    if (visible && job.slots > 0) HIP_CHECK(hipMemsetAsync(visible, 0, (size_t)job.n_images * job.slots * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_rle_draw<RD_MAP>, rd_grid(job, job.n_images), dim3(256), 0, s, job, reinterpret_cast<uint8_t*>(map), visible, nullptr, 0, 0, 0);
    HIP_CHECK(hipGetLastError());
}

void render_detections_rle_forward(hipStream_t s, const RleDrawJob& job, const uint8_t* const* srcs, int alpha, int stroke, uint8_t* out)
{
    if (job.n_images <= 0) return;
    hipLaunchKernelGGL(k_rle_draw<RD_RENDER>, rd_grid(job, job.n_images), dim3(256), 0, s, job, out, nullptr, srcs, alpha, stroke / 2,
                       stroke - stroke / 2);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
