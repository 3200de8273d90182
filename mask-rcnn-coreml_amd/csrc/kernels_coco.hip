// kernels_coco.hip — COCO scoring on the device: RLE x RLE intersection, box IoU, and COCOeval's greedy matching.
// Built with -ffp-contract=off like the box kernels: the IoU quotients are plain IEEE double operations, one rounding each.
//
// An RLE is a range of `counts` (uint32 run lengths, column-major pixels, counts[0] = leading zeros, then ones / zeros alternating):
// RLE k owns counts[run_offsets[k] .. run_offsets[k+1]) — the layout mrcnn_masks_rle_source writes.
//
// Intersection without walking the two run lists in lockstep.  With B[j] the exclusive prefix sum of an RLE's counts (the pixel
// position where run j starts) and O[j] the set pixels before run j, the set pixels before position p are
//     G(p) = O[j] + (j odd ? p - B[j] : 0),   j = the last run with B[j] <= p            (a binary search in B)
// and   inter(d, g) = sum over d's ones-runs [s, e) of G_g(e) - G_g(s).   Integer arithmetic: exact in any order of summation.
#include "kernels.h"

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

// One block per RLE: B (exclusive prefix of the counts) and O (exclusive prefix of the odd runs) into `pre` (either may be nullptr: only
// the sums are wanted), the pixel count into totals[k] and the set pixels into areas[k].  Runs are taken 256 at a time with a carry.
__global__ __launch_bounds__(256) void k_rle_prefix(const uint32_t* __restrict__ counts, const long long* __restrict__ run_offsets, long n_rle,
                                                    uint32_t* __restrict__ pre_b, uint32_t* __restrict__ pre_o,
                                                    unsigned long long* __restrict__ totals, uint32_t* __restrict__ areas)
{
    const long k = blockIdx.x;
    if (k >= n_rle) return;
    const long long r0 = run_offsets[k], r1 = run_offsets[k + 1];
    __shared__ unsigned long long sh_b[256 / WAVE];
    __shared__ unsigned long long sh_o[256 / WAVE];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    unsigned long long carry_b = 0, carry_o = 0;
    for (long long base = r0; base < r1; base += 256) {
        const long long j = base + threadIdx.x;
        const unsigned long long c = j < r1 ? counts[j] : 0u;
        const unsigned long long o = ((j - r0) & 1) ? c : 0u;
        unsigned long long sb = c, so = o;                      // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long tb = __shfl_up(sb, d, WAVE), to = __shfl_up(so, d, WAVE);
            if (lane >= d) { sb += tb; so += to; }
        }
        if (lane == WAVE - 1) { sh_b[wave] = sb; sh_o[wave] = so; }
        __syncthreads();
        unsigned long long wb = 0, wo = 0, all_b = 0, all_o = 0;
#pragma unroll
        for (int w = 0; w < 256 / WAVE; ++w) {
            if (w < wave) { wb += sh_b[w]; wo += sh_o[w]; }
            all_b += sh_b[w]; all_o += sh_o[w];
        }
        if (j < r1) {
            if (pre_b) pre_b[j] = (uint32_t)(carry_b + wb + sb - c);
            if (pre_o) pre_o[j] = (uint32_t)(carry_o + wo + so - o);
        }
        carry_b += all_b; carry_o += all_o;
        __syncthreads();
    }
    if (threadIdx.x == 0) { totals[k] = carry_b; areas[k] = (uint32_t)carry_o; }
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

}  // namespace

void rle_prefix_forward(hipStream_t s, const uint32_t* counts, const long long* run_offsets, long n_rle, uint32_t* pre_b, uint32_t* pre_o,
                        unsigned long long* totals, uint32_t* areas)
{
    if (n_rle <= 0) return;
    hipLaunchKernelGGL(k_rle_prefix, dim3((unsigned)n_rle), dim3(256), 0, s, counts, run_offsets, n_rle, pre_b, pre_o, totals, areas);
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
