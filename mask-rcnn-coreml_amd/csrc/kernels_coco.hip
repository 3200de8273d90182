// kernels_coco.hip — COCO scoring on the device: RLE x RLE intersection, box IoU, COCOeval's greedy matching, and polygon ground
// truth to RLE.  Built with -ffp-contract=off like the box kernels: the IoU quotients and the polygon arithmetic are plain IEEE double
// operations, one rounding each.
//
// An RLE is a range of `counts` (uint32 run lengths, column-major pixels, counts[0] = leading zeros, then ones / zeros alternating):
// RLE k owns counts[run_offsets[k] .. run_offsets[k+1]) — the layout mrcnn_masks_rle_source writes.
//
// Intersection without walking the two run lists in lockstep (the tables: k_rle_prefix, kernels_rle_prefix.hip, shared with the RLE
// drawing kernels).  With B[j] the exclusive prefix sum of an RLE's counts (the pixel
// position where run j starts) and O[j] the set pixels before run j, the set pixels before position p are
//     G(p) = O[j] + (j odd ? p - B[j] : 0),   j = the last run with B[j] <= p            (a binary search in B)
// and   inter(d, g) = sum over d's ones-runs [s, e) of G_g(e) - G_g(s).   Integer arithmetic: exact in any order of summation.
#include <vector>

#include "kernels.h"
#include "poly_device.h"

namespace mrcnn {
namespace {

constexpr int WAVE = 64;
constexpr int IOU_BLOCK = 256;                    // 4 waves: 4 detections against ONE ground truth, whose tables they share in LDS
constexpr int IOU_WAVES = IOU_BLOCK / WAVE;
constexpr int IOU_LDS_RUNS = 2048;                // ground-truth runs staged per block: 2 tables x 2048 x 4 B = 16 KiB -> 10 blocks per CU (160 KiB)

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// set pixels of the ground truth before position p: tb / to are its B / O tables (LDS or global), n its number of runs (>= 1)
__device__ __forceinline__ uint32_t ones_before(const uint32_t* tb, const uint32_t* to, int n, uint32_t p)
{
    int lo = 0, hi = n - 1;                                  // B[0] = 0 <= p: the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return to[lo] + ((lo & 1) ? p - tb[lo] : 0u);
}

__device__ __forceinline__ int find_group(const long long* __restrict__ starts, int n_groups, long long b)
{
    int lo = 0, hi = n_groups - 1;                           // the last group with starts[group] <= b (empty groups repeat a start)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The grid is the sum over the groups of ceil(nd / 4) * ng blocks (block_starts: its prefix, n_groups + 1 entries): block = 4 detections
// x 1 ground truth of one image, one wave per pair, lanes striding the detection's ones-runs.
__global__ __launch_bounds__(IOU_BLOCK) void k_rle_iou(const uint32_t* __restrict__ d_b, const long long* __restrict__ d_off,
                                                       const unsigned long long* __restrict__ d_total, const uint32_t* __restrict__ d_area,
                                                       const uint32_t* __restrict__ g_b, const uint32_t* __restrict__ g_o,
                                                       const long long* __restrict__ g_off, const uint32_t* __restrict__ g_area,
                                                       const uint8_t* __restrict__ g_crowd, const IouGroup* __restrict__ groups,
                                                       const long long* __restrict__ block_starts, int n_groups,
                                                       uint32_t* __restrict__ inter_out, double* __restrict__ iou_out)
{
    __shared__ uint32_t sh_b[IOU_LDS_RUNS];
    __shared__ uint32_t sh_o[IOU_LDS_RUNS];
    const long long blk = blockIdx.x;
    const int gi = find_group(block_starts, n_groups, blk);
    const IouGroup G = groups[gi];
    const long long nd = G.d1 - G.d0, ng = G.g1 - G.g0;
    const long long local = blk - block_starts[gi];
    const long long g_local = local % ng, d_tile = local / ng;
    const long long g = G.g0 + g_local;
    const long long gr0 = g_off[g];
    const int gn = (int)(g_off[g + 1] - gr0);
    const bool staged = gn <= IOU_LDS_RUNS;
    if (staged) {
        for (int i = threadIdx.x; i < gn; i += IOU_BLOCK) { sh_b[i] = g_b[gr0 + i]; sh_o[i] = g_o[gr0 + i]; }
        __syncthreads();
    }
    const uint32_t* tb = staged ? sh_b : g_b + gr0;
    const uint32_t* to = staged ? sh_o : g_o + gr0;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long long d_local = d_tile * IOU_WAVES + wave;
    if (d_local >= nd) return;                                // (behind the only barrier)
    const long long d = G.d0 + d_local;
    const long long dr0 = d_off[d], dr1 = d_off[d + 1];
    const uint32_t total = (uint32_t)d_total[d];             // == the ground truth's (checked on the host before the launch)
    uint32_t acc = 0;
    if (g_area[g] != 0)
        for (long long j = dr0 + 1 + 2 * (long long)lane; j < dr1; j += 2 * WAVE) {        // the odd runs are the ones: [s, e)
            const uint32_t s = d_b[j];
            const uint32_t e = j + 1 < dr1 ? d_b[j + 1] : total;
            if (e > s) acc += ones_before(tb, to, gn, e) - ones_before(tb, to, gn, s);
        }
    acc = wave_sum_u32(acc);
    if (lane == 0) {
        const long long o = G.out_offset + d_local * ng + g_local;
        const uint32_t ad = d_area[d], ag = g_area[g];
        const unsigned long long den = g_crowd[g] ? (unsigned long long)ad : (unsigned long long)ad + ag - acc;
        if (inter_out) inter_out[o] = acc;
        if (iou_out) iou_out[o] = den ? (double)acc / (double)den : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_box_iou_xywh(const double* __restrict__ db, const double* __restrict__ gb, const uint8_t* __restrict__ g_crowd,
                                                      const IouGroup* __restrict__ groups, const long long* __restrict__ pair_starts, int n_groups,
                                                      long long n_pairs, double* __restrict__ iou_out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int gi = find_group(pair_starts, n_groups, p);
    const IouGroup G = groups[gi];
    const long long ng = G.g1 - G.g0, local = p - pair_starts[gi];
    const long long d = G.d0 + local / ng, g = G.g0 + local % ng;
    const double* D = db + 4 * d;
    const double* T = gb + 4 * g;
    const double da = D[2] * D[3], ga = T[2] * T[3];
    double o = 0.0;
    const double w = fmin(D[2] + D[0], T[2] + T[0]) - fmax(D[0], T[0]);
    const double h = fmin(D[3] + D[1], T[3] + T[1]) - fmax(D[1], T[1]);
    if (w > 0.0 && h > 0.0) {
        const double i = w * h;
        const double u = g_crowd[g] ? da : da + ga - i;
        o = u != 0.0 ? i / u : 0.0;
    }
    iou_out[G.out_offset + local] = o;
}

// COCOeval.evaluateImg's greedy pass: one wave per (match group, area range a, threshold t).  The detections (score order) are taken
// one after the other; the scan over the group's ground truths is a wave-wide arg-max.  The order "non-ignored first, stable" is two
// passes over the list — first the non-ignored, then the ignored — each in list order: inside a pass the later of equal IoUs wins,
// and the ignored are only looked at when no non-ignored one was taken.  The lane that owns a ground truth (j % 64) is the only one
// that reads or writes its state.
__global__ __launch_bounds__(WAVE) void k_coco_match(const double* __restrict__ iou, const MatchGroup* __restrict__ groups, int n_groups,
                                                     const int32_t* __restrict__ dt_idx, const double* __restrict__ dt_area,
                                                     const int32_t* __restrict__ gt_idx, const double* __restrict__ gt_area,
                                                     const uint8_t* __restrict__ gt_crowd, const double* __restrict__ ranges, int A,
                                                     const double* __restrict__ thrs, int T, int32_t* __restrict__ dt_match,
                                                     uint8_t* __restrict__ dt_ignore, int32_t* __restrict__ gt_match)
{
    const long long w = blockIdx.x;
    const int t = (int)(w % T), a = (int)((w / T) % A);
    const long long k = w / ((long long)T * A);
    if (k >= n_groups) return;
    const MatchGroup G = groups[k];
    const int nd = G.dt1 - G.dt0, ng = G.gt1 - G.gt0;
    const int lane = threadIdx.x;
    const double lo = ranges[2 * a], hi = ranges[2 * a + 1];
    const double bar0 = fmin(thrs[t], 1.0 - 1e-10);
    const long long AT = (long long)A * T, at = (long long)a * T + t;
    int32_t* gm = gt_match + AT * G.gt0 + at * ng;
    int32_t* dm = dt_match + AT * G.dt0 + at * nd;
    uint8_t* di = dt_ignore + AT * G.dt0 + at * nd;
    for (int j = lane; j < ng; j += WAVE) gm[j] = -1;
    for (int i = 0; i < nd; ++i) {
        const double* row = iou + G.iou_offset + (long long)dt_idx[G.dt0 + i] * G.iou_stride;
        int m = -1, m_ig = 0;
        for (int pass = 0; pass < 2 && m < 0; ++pass) {
            double best = -1.0;
            int bj = -1;
            for (int j = lane; j < ng; j += WAVE) {
                const int q = G.gt0 + j;
                const bool crowd = gt_crowd[q] != 0;
                const double ar = gt_area[q];
                const int ig = (crowd || ar < lo || ar > hi) ? 1 : 0;
                if (ig != pass) continue;
                if (gm[j] >= 0 && !crowd) continue;
                const double v = row[gt_idx[q]];
                if (v < bar0) continue;
                if (v >= best) { best = v; bj = j; }                 // the lane's own indices ascend: the later of equals
            }
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, WAVE);
                const int oj = __shfl_xor(bj, o, WAVE);
                if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj > bj))) { best = ob; bj = oj; }
            }
            if (bj >= 0) { m = bj; m_ig = pass; }
        }
        if (m >= 0 && (m % WAVE) == lane) gm[m] = i;
        if (lane == 0) {
            const double ar = dt_area[G.dt0 + i];
            dm[i] = m;
            di[i] = m >= 0 ? (uint8_t)m_ig : (uint8_t)((ar < lo || ar > hi) ? 1 : 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Polygon ground truth -> RLE (mrcnn_rle_from_polygons_batch).  The host entry mrcnn_rle_from_polygons is the specification; its
// arithmetic, in closed form per (edge, pixel column), is poly_device.h.  What is parallel here:
//   k_poly_edge_count   one thread per edge: how many column centres it crosses
//   k_poly_scan         exclusive prefix of uint32 -> int64 (one block, 8192 entries per step); used for the edges and for the runs
//   k_poly_encode_lds   one block per annotation whose toggles fit LDS.  A thread owns toggle q, finds its edge by bisection in the
//                       prefix and evaluates it.  Key 1 = (polygon << 32 | position): after a bitonic sort the rank of a toggle inside
//                       its polygon is its index minus the polygon's first, and its parity says whether the toggle opens (+1) or
//                       closes (-1) an interval — equal positions cancel, a trailing opener stays open to the end of the plane.
//                       Key 2 = (position << 1 | closes): after the second sort the inclusive prefix of the signs is the coverage
//                       count of the annotation; a position is a run boundary when "covered" differs before and behind ALL events at
//                       it — the host's union of touching intervals (`first <= e`).  Boundaries are compacted in order.
//   k_poly_*_big        the same steps for an annotation with more toggles, its keys in global memory: generation, pairing and union
//                       by one block per annotation, the two sorts as grid-wide bitonic steps over all such annotations at once.
//   k_poly_write        run r = boundary r - boundary r-1, closed by the run to h*w.
// ------------------------------------------------------------------------------------------------
constexpr int POLY_BLOCK = 256;
constexpr int POLY_BIG_BLOCK = 1024;
constexpr int POLY_SCAN_ITEMS = 8;
typedef unsigned long long u64;

// inclusive scan over the block (up to 16 waves); `sh` holds 16 entries and is free again on return
template <class T>
__device__ __forceinline__ T poly_block_scan(T v, T* sh, T& total)
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, nw = (blockDim.x + WAVE - 1) / WAVE;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T t = __shfl_up(v, d, WAVE);
        if (lane >= d) v += t;
    }
    if (lane == WAVE - 1) sh[wave] = v;
    __syncthreads();
    T add = 0, tot = 0;
    for (int w = 0; w < nw; ++w) { const T x = sh[w]; if (w < wave) add += x; tot += x; }
    __syncthreads();
    total = tot;
    return v + add;
}

__device__ __forceinline__ PolyEdge poly_edge_at(const double* __restrict__ xy, const PolyRec P, long long e, int w)
{
    const long long nx = e + 1 == P.pt0 + P.npts ? P.pt0 : e + 1;
    return poly_edge(poly_quant(xy[2 * e]), poly_quant(xy[2 * e + 1]), poly_quant(xy[2 * nx]), poly_quant(xy[2 * nx + 1]), w);
}

__global__ __launch_bounds__(256) void k_poly_edge_count(const double* __restrict__ xy, const int32_t* __restrict__ pt_poly,
                                                         const PolyRec* __restrict__ polys, const PolyAnn* __restrict__ anns, long n_pts,
                                                         uint32_t* __restrict__ edge_cnt)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pts) return;
    const PolyRec P = polys[pt_poly[e]];
    edge_cnt[e] = (uint32_t)poly_edge_at(xy, P, e, anns[P.ann].w).cnt;
}

// out[i] = sum of in[0 .. i), out[n] = the sum; one block of 1024 threads, 8 consecutive entries per thread and step
__global__ __launch_bounds__(1024) void k_poly_scan(const uint32_t* __restrict__ in, long n, long long* __restrict__ out)
{
    __shared__ long long sh[16];
    long long carry = 0;
    const long step = 1024L * POLY_SCAN_ITEMS;
    for (long base = 0; base < n; base += step) {
        const long at = base + (long)threadIdx.x * POLY_SCAN_ITEMS;
        uint32_t v[POLY_SCAN_ITEMS];
        long long mine = 0;
#pragma unroll
        for (int i = 0; i < POLY_SCAN_ITEMS; ++i) { v[i] = at + i < n ? in[at + i] : 0u; mine += v[i]; }
        long long tot;
        long long run = carry + poly_block_scan<long long>(mine, sh, tot) - mine;
#pragma unroll
        for (int i = 0; i < POLY_SCAN_ITEMS; ++i) { if (at + i < n) out[at + i] = run; run += v[i]; }
        carry += tot;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(256) void k_poly_gather(const long long* __restrict__ edge_start, const PolyAnn* __restrict__ anns, long n_anns,
                                                     long n_pts, long long* __restrict__ tog_off)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_anns) tog_off[k] = edge_start[anns[k].pt0];
    else if (k == n_anns) tog_off[k] = edge_start[n_pts];
}

// keys[q] = (polygon of the annotation << 32 | position) of toggle q of annotation A for q < m, all ones for m <= q < padded
__device__ __forceinline__ void poly_generate(const double* __restrict__ xy, const int32_t* __restrict__ pt_poly, const PolyRec* __restrict__ polys,
                                              const PolyAnn A, const long long* __restrict__ edge_start, long long m, long long padded, u64* keys)
{
    const long long base = edge_start[A.pt0];
    for (long long q = threadIdx.x; q < padded; q += blockDim.x) {
        u64 key = ~0ull;
        if (q < m) {
            long long lo = A.pt0, hi = A.pt1 - 1;               // the last edge with edge_start[e] - base <= q (edges without toggles repeat a start)
            while (lo < hi) {
                const long long mid = (lo + hi + 1) >> 1;
                if (edge_start[mid] - base <= q) lo = mid; else hi = mid - 1;
            }
            const int p = pt_poly[lo];
            const PolyEdge e = poly_edge_at(xy, polys[p], lo, A.w);
            const int c = (int)(q - (edge_start[lo] - base));
            key = ((u64)(uint32_t)(p - A.poly0) << 32) | poly_toggle(e, e.klo + c, A.h);
        }
        keys[q] = key;
    }
}

// one compare-exchange of the bitonic network on keys[0 .. padded): pair i of step (k, j)
__device__ __forceinline__ void poly_bitonic_pair(u64* keys, long long i, long long k, long long j)
{
    const long long lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
    const u64 x = keys[lo], y = keys[hi];
    if ((x > y) == ((lo & k) == 0)) { keys[lo] = y; keys[hi] = x; }
}

__device__ __forceinline__ void poly_block_sort(u64* keys, long long padded)
{
    for (long long k = 2; k <= padded; k <<= 1)
        for (long long j = k >> 1; j > 0; j >>= 1) {
            for (long long i = threadIdx.x; i < padded / 2; i += blockDim.x) poly_bitonic_pair(keys, i, k, j);
            __syncthreads();
        }
}

// sorted key 1 -> key 2 in place: the rank of a toggle inside its polygon decides its sign
__device__ __forceinline__ void poly_pair(const PolyRec* __restrict__ polys, const PolyAnn A, const long long* __restrict__ edge_start, long long m, u64* keys)
{
    const long long base = edge_start[A.pt0];
    for (long long q = threadIdx.x; q < m; q += blockDim.x) {
        const u64 key = keys[q];
        const long long first = edge_start[polys[A.poly0 + (int)(key >> 32)].pt0] - base;
        keys[q] = ((key & 0xffffffffull) << 1) | (u64)((q - first) & 1);
    }
}

// sorted key 2 -> the run boundaries in order (bnd, at most m), their number, and from them the runs, the area and the tight box.
// cov (m entries) is scratch.  sh: 16 long long.  Every thread of the block calls this; ends behind a barrier.
__device__ __forceinline__ void poly_unite(const u64* keys, int32_t* cov, long long m, const PolyAnn A, uint32_t* __restrict__ bnd, long long k,
                                           uint32_t* __restrict__ nb_out, uint32_t* __restrict__ nruns, uint32_t* __restrict__ areas,
                                           int32_t* __restrict__ bboxes, long long* sh)
{
    int carry = 0;
    for (long long b0 = 0; b0 < m; b0 += blockDim.x) {           // coverage behind every event
        const long long i = b0 + threadIdx.x;
        const int v = i < m ? ((keys[i] & 1) ? -1 : 1) : 0;
        int tot;
        const int incl = poly_block_scan<int>(v, reinterpret_cast<int*>(sh), tot);
        if (i < m) cov[i] = carry + incl;
        carry += tot;
    }
    __syncthreads();
    long long nb = 0;
    for (long long b0 = 0; b0 < m; b0 += blockDim.x) {           // the last event of every position decides; compact the boundaries
        const long long i = b0 + threadIdx.x;
        int flag = 0;
        uint32_t pos = 0;
        if (i < m) {
            const u64 key = keys[i];
            pos = (uint32_t)(key >> 1);
            if (i == m - 1 || (uint32_t)(keys[i + 1] >> 1) != pos) {
                const u64 bar = key & ~1ull;                     // the first event at this position: lower bound of (pos << 1)
                long long lo = 0, hi = i;
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (keys[mid] >= bar) hi = mid; else lo = mid + 1;
                }
                const int before = lo > 0 ? cov[lo - 1] : 0;
                flag = (cov[i] > 0) != (before > 0);
            }
        }
        long long tot;
        const long long incl = poly_block_scan<long long>((long long)flag, sh, tot);
        if (flag) bnd[nb + incl - 1] = pos;
        nb += tot;
    }
    __syncthreads();                                             // the block's own stores to bnd are visible to it
    const uint32_t total = (uint32_t)A.h * (uint32_t)A.w;
    const uint32_t last = nb ? bnd[nb - 1] : 0u;
    // the ones-runs [bnd[2r], bnd[2r + 1]), the last one open to the end of the plane
    long long area = 0;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (long long r = threadIdx.x; 2 * r < nb; r += blockDim.x) {
        const uint32_t s = bnd[2 * r], e = 2 * r + 1 < nb ? bnd[2 * r + 1] : total;
        if (e <= s) continue;
        area += e - s;
        const int x0 = (int)(s / (uint32_t)A.h), x1 = (int)((e - 1) / (uint32_t)A.h);
        const int y0 = x1 > x0 ? 0 : (int)(s % (uint32_t)A.h), y1 = x1 > x0 ? A.h - 1 : (int)((e - 1) % (uint32_t)A.h);
        xmin = min(xmin, x0); xmax = max(xmax, x1); ymin = min(ymin, y0); ymax = max(ymax, y1);
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        area += __shfl_xor(area, o, WAVE);
        xmin = min(xmin, __shfl_xor(xmin, o, WAVE)); ymin = min(ymin, __shfl_xor(ymin, o, WAVE));
        xmax = max(xmax, __shfl_xor(xmax, o, WAVE)); ymax = max(ymax, __shfl_xor(ymax, o, WAVE));
    }
    __shared__ int s_box[16][4];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, nw = (blockDim.x + WAVE - 1) / WAVE;
    if (lane == 0) { sh[wave] = area; s_box[wave][0] = xmin; s_box[wave][1] = ymin; s_box[wave][2] = xmax; s_box[wave][3] = ymax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) {
            area += sh[w];
            xmin = min(xmin, s_box[w][0]); ymin = min(ymin, s_box[w][1]); xmax = max(xmax, s_box[w][2]); ymax = max(ymax, s_box[w][3]);
        }
        nb_out[k] = (uint32_t)nb;
        nruns[k] = (uint32_t)nb + ((nb == 0 || last < total) ? 1u : 0u);
        if (areas) areas[k] = (uint32_t)area;
        if (bboxes) {
            int* o = bboxes + 4 * k;
            const bool any = area > 0;
            o[0] = any ? xmin : 0; o[1] = any ? ymin : 0; o[2] = any ? xmax - xmin + 1 : 0; o[3] = any ? ymax - ymin + 1 : 0;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ long long poly_pow2(long long m)
{
    long long p = 1;
    while (p < m) p <<= 1;
    return p;
}

__global__ __launch_bounds__(POLY_BLOCK) void k_poly_encode_lds(const double* __restrict__ xy, const int32_t* __restrict__ pt_poly,
                                                                const PolyRec* __restrict__ polys, const PolyAnn* __restrict__ anns,
                                                                const long long* __restrict__ edge_start, uint32_t* __restrict__ bnd,
                                                                uint32_t* __restrict__ nb, uint32_t* __restrict__ nruns,
                                                                uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes)
{
    __shared__ u64 keys[POLY_LDS_TOGGLES];
    __shared__ int32_t cov[POLY_LDS_TOGGLES];
    __shared__ long long sh[16];
    const long long k = blockIdx.x;
    const PolyAnn A = anns[k];
    const long long base = edge_start[A.pt0], m = edge_start[A.pt1] - base;
    if (m > POLY_LDS_TOGGLES) return;                             // (the whole block: this annotation goes the global way)
    const long long padded = poly_pow2(m);
    poly_generate(xy, pt_poly, polys, A, edge_start, m, padded, keys);
    __syncthreads();
    poly_block_sort(keys, padded);
    poly_pair(polys, A, edge_start, m, keys);
    __syncthreads();
    poly_block_sort(keys, padded);
    poly_unite(keys, cov, m, A, bnd + base, k, nb, nruns, areas, bboxes, sh);
}

__global__ __launch_bounds__(POLY_BIG_BLOCK) void k_poly_generate_big(const double* __restrict__ xy, const int32_t* __restrict__ pt_poly,
                                                                      const PolyRec* __restrict__ polys, const PolyAnn* __restrict__ anns,
                                                                      const long long* __restrict__ edge_start, const PolyBig* __restrict__ big,
                                                                      u64* __restrict__ keys)
{
    const PolyBig B = big[blockIdx.x];
    const PolyAnn A = anns[B.ann];
    poly_generate(xy, pt_poly, polys, A, edge_start, edge_start[A.pt1] - edge_start[A.pt0], B.padded, keys + B.offset);
}

// step (k, j) of the bitonic network over every listed annotation whose padded size reaches k; pair_start = prefix of padded / 2
__global__ __launch_bounds__(256) void k_poly_bitonic_big(const PolyBig* __restrict__ big, const long long* __restrict__ pair_start, int n_big,
                                                          long long n_pairs, long long k, long long j, u64* __restrict__ keys)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_pairs) return;
    const int b = find_group(pair_start, n_big, g);
    const PolyBig B = big[b];
    if (B.padded < k) return;
    poly_bitonic_pair(keys + B.offset, g - pair_start[b], k, j);
}

__global__ __launch_bounds__(POLY_BIG_BLOCK) void k_poly_pair_big(const PolyRec* __restrict__ polys, const PolyAnn* __restrict__ anns,
                                                                  const long long* __restrict__ edge_start, const PolyBig* __restrict__ big,
                                                                  u64* __restrict__ keys)
{
    const PolyBig B = big[blockIdx.x];
    const PolyAnn A = anns[B.ann];
    poly_pair(polys, A, edge_start, edge_start[A.pt1] - edge_start[A.pt0], keys + B.offset);
}

__global__ __launch_bounds__(POLY_BIG_BLOCK) void k_poly_unite_big(const PolyAnn* __restrict__ anns, const long long* __restrict__ edge_start,
                                                                   const PolyBig* __restrict__ big, const u64* __restrict__ keys,
                                                                   int32_t* __restrict__ cov, uint32_t* __restrict__ bnd, uint32_t* __restrict__ nb,
                                                                   uint32_t* __restrict__ nruns, uint32_t* __restrict__ areas,
                                                                   int32_t* __restrict__ bboxes)
{
    __shared__ long long sh[16];
    const PolyBig B = big[blockIdx.x];
    const PolyAnn A = anns[B.ann];
    const long long base = edge_start[A.pt0];
    poly_unite(keys + B.offset, cov + B.offset, edge_start[A.pt1] - base, A, bnd + base, B.ann, nb, nruns, areas, bboxes, sh);
}

__global__ __launch_bounds__(POLY_BLOCK) void k_poly_write(const PolyAnn* __restrict__ anns, const long long* __restrict__ tog_off,
                                                           const uint32_t* __restrict__ bnd, const uint32_t* __restrict__ nb,
                                                           const long long* __restrict__ run_offsets, uint32_t* __restrict__ counts)
{
    const long long k = blockIdx.x;
    const uint32_t* b = bnd + tog_off[k];
    const long long n = nb[k], r0 = run_offsets[k], r1 = run_offsets[k + 1];
    for (long long r = threadIdx.x; r < n; r += blockDim.x) counts[r0 + r] = b[r] - (r ? b[r - 1] : 0u);
    if (threadIdx.x == 0 && r1 - r0 > n) counts[r0 + n] = (uint32_t)anns[k].h * (uint32_t)anns[k].w - (n ? b[n - 1] : 0u);
}

}  // namespace

void poly_count_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns, long n_pts, long n_anns,
                        uint32_t* edge_cnt, long long* edge_start, long long* tog_off)
{
    if (n_pts > 0) {
        hipLaunchKernelGGL(k_poly_edge_count, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, s, xy, pt_poly, polys, anns, n_pts, edge_cnt);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_poly_scan, dim3(1), dim3(1024), 0, s, edge_cnt, n_pts, edge_start);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_poly_gather, dim3((unsigned)((n_anns + 1 + 255) / 256)), dim3(256), 0, s, edge_start, anns, n_anns, n_pts, tog_off);
    HIP_CHECK(hipGetLastError());
}

void poly_encode_lds_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns, long n_anns,
                             const long long* edge_start, uint32_t* bnd, uint32_t* nb, uint32_t* nruns, uint32_t* areas, int32_t* bboxes)
{
    if (n_anns <= 0) return;
    hipLaunchKernelGGL(k_poly_encode_lds, dim3((unsigned)n_anns), dim3(POLY_BLOCK), 0, s, xy, pt_poly, polys, anns, edge_start, bnd, nb, nruns, areas,
                       bboxes);
    HIP_CHECK(hipGetLastError());
}

void poly_encode_big_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns,
                             const long long* edge_start, const PolyBig* big, const PolyBig* h_big, int n_big, unsigned long long* keys, int32_t* cov,
                             uint32_t* bnd, uint32_t* nb, uint32_t* nruns, uint32_t* areas, int32_t* bboxes)
{
    if (n_big <= 0) return;
    std::vector<long long> starts((size_t)n_big + 1, 0);
    long long widest = 1;
    for (int b = 0; b < n_big; ++b) {
        starts[(size_t)b + 1] = starts[(size_t)b] + h_big[b].padded / 2;
        widest = h_big[b].padded > widest ? h_big[b].padded : widest;
    }
    const long long n_pairs = starts[(size_t)n_big];
    DevBuf ps(starts.size() * 8);
    HIP_CHECK(hipMemcpyAsync(ps.p, starts.data(), starts.size() * 8, hipMemcpyHostToDevice, s));
    auto sort_all = [&] {
        for (long long k = 2; k <= widest; k <<= 1)
            for (long long j = k >> 1; j > 0; j >>= 1)
                hipLaunchKernelGGL(k_poly_bitonic_big, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, big, ps.as<long long>(), n_big, n_pairs,
                                   k, j, keys);
        HIP_CHECK(hipGetLastError());
    };
    hipLaunchKernelGGL(k_poly_generate_big, dim3((unsigned)n_big), dim3(POLY_BIG_BLOCK), 0, s, xy, pt_poly, polys, anns, edge_start, big, keys);
    HIP_CHECK(hipGetLastError());
    sort_all();
    hipLaunchKernelGGL(k_poly_pair_big, dim3((unsigned)n_big), dim3(POLY_BIG_BLOCK), 0, s, polys, anns, edge_start, big, keys);
    HIP_CHECK(hipGetLastError());
    sort_all();
    hipLaunchKernelGGL(k_poly_unite_big, dim3((unsigned)n_big), dim3(POLY_BIG_BLOCK), 0, s, anns, edge_start, big, keys, cov, bnd, nb, nruns, areas, bboxes);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                         // `starts` on the host and `ps` are read by the launches above
}

void poly_offsets_forward(hipStream_t s, const uint32_t* nruns, long n, long long* run_offsets)
{
    hipLaunchKernelGGL(k_poly_scan, dim3(1), dim3(1024), 0, s, nruns, n, run_offsets);
    HIP_CHECK(hipGetLastError());
}

void poly_write_forward(hipStream_t s, const PolyAnn* anns, long n_anns, const long long* tog_off, const uint32_t* bnd, const uint32_t* nb,
                        const long long* run_offsets, uint32_t* counts)
{
    if (n_anns <= 0) return;
    hipLaunchKernelGGL(k_poly_write, dim3((unsigned)n_anns), dim3(POLY_BLOCK), 0, s, anns, tog_off, bnd, nb, run_offsets, counts);
    HIP_CHECK(hipGetLastError());
}

void rle_iou_forward(hipStream_t s, const uint32_t* d_b, const long long* d_off, const unsigned long long* d_total, const uint32_t* d_area, const uint32_t* g_b, const uint32_t* g_o,
                     const long long* g_off, const uint32_t* g_area, const uint8_t* g_crowd, const IouGroup* groups, const long long* block_starts,
                     int n_groups, long long n_blocks, uint32_t* inter, double* iou)
{
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(k_rle_iou, dim3((unsigned)n_blocks), dim3(IOU_BLOCK), 0, s, d_b, d_off, d_total, d_area, g_b, g_o, g_off, g_area, g_crowd, groups,
                       block_starts, n_groups, inter, iou);
    HIP_CHECK(hipGetLastError());
}

void box_iou_xywh_forward(hipStream_t s, const double* db, const double* gb, const uint8_t* g_crowd, const IouGroup* groups,
                          const long long* pair_starts, int n_groups, long long n_pairs, double* iou)
{
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(k_box_iou_xywh, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, db, gb, g_crowd, groups, pair_starts, n_groups,
                       n_pairs, iou);
    HIP_CHECK(hipGetLastError());
}

void coco_match_forward(hipStream_t s, const double* iou, const MatchGroup* groups, int n_groups, const int32_t* dt_idx, const double* dt_area,
                        const int32_t* gt_idx, const double* gt_area, const uint8_t* gt_crowd, const double* ranges, int A, const double* thrs, int T,
                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match)
{
    const long long waves = (long long)n_groups * A * T;
    if (waves <= 0) return;
    hipLaunchKernelGGL(k_coco_match, dim3((unsigned)waves), dim3(WAVE), 0, s, iou, groups, n_groups, dt_idx, dt_area, gt_idx, gt_area, gt_crowd,
                       ranges, A, thrs, T, dt_match, dt_ignore, gt_match);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
