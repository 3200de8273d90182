// kernels_rle_prefix.hip — the prefix tables of a set of run-length masks, shared by COCO scoring (kernels_coco.hip's intersection walks
// them) and by the RLE drawing kernels (kernels_rle_draw.hip finds the run that holds a pixel position in them).
//
// An RLE is a range of `counts` (uint32 run lengths, column-major pixels, counts[0] = leading zeros, then ones / zeros alternating):
// RLE k owns counts[run_offsets[k] .. run_offsets[k+1]).  B[j] is the exclusive prefix sum of its counts (the position where run j
// starts), O[j] the set pixels before run j.  Algorithmic bytes: 4 read + 4 (B) [+ 4 (O)] written per run.
#include "kernels.h"

namespace mrcnn {
namespace {

constexpr int WAVE = 64;

// One block per RLE: B (exclusive prefix of the counts) and O (exclusive prefix of the odd runs) into `pre` (either may be nullptr: only
// the sums are wanted), the pixel count into totals[k] and the set pixels into areas[k].  Runs are taken 256 at a time with a carry.
// extent[k] (may be nullptr) = (first, last): the positions of the RLE's first and last set pixel, (0xffffffff, 0) when it has none.
__global__ __launch_bounds__(256) void k_rle_prefix(const uint32_t* __restrict__ counts, const long long* __restrict__ run_offsets, long n_rle,
                                                    uint32_t* __restrict__ pre_b, uint32_t* __restrict__ pre_o,
                                                    unsigned long long* __restrict__ totals, uint32_t* __restrict__ areas, uint2* __restrict__ extent)
{
    const long k = blockIdx.x;
    if (k >= n_rle) return;
    const long long r0 = run_offsets[k], r1 = run_offsets[k + 1];
    __shared__ unsigned long long sh_b[256 / WAVE];
    __shared__ unsigned long long sh_o[256 / WAVE];
    __shared__ uint32_t sh_first, sh_last;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) { sh_first = 0xffffffffu; sh_last = 0u; }
    unsigned long long carry_b = 0, carry_o = 0;
    unsigned long long first = 0xffffffffull, last = 0;      // of this thread's ones-runs (64 bit: a bad RLE may sum past 2^32)
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
            const unsigned long long start = carry_b + wb + sb - c;
            if (pre_b) pre_b[j] = (uint32_t)start;
            if (pre_o) pre_o[j] = (uint32_t)(carry_o + wo + so - o);
            if (o) {
                first = start < first ? start : first;
                last = start + c - 1 > last ? start + c - 1 : last;
            }
        }
        carry_b += all_b; carry_o += all_o;
        __syncthreads();
    }
    if (threadIdx.x == 0) { totals[k] = carry_b; areas[k] = (uint32_t)carry_o; }
    if (extent) {                                               // (uniform: the barriers below are reached by all or none)
        __syncthreads();                                        // (an RLE without runs passed no barrier since sh_first was set)
        if (first <= last) {
            atomicMin(&sh_first, (uint32_t)(first > 0xffffffffull ? 0xffffffffull : first));
            atomicMax(&sh_last, (uint32_t)(last > 0xffffffffull ? 0xffffffffull : last));
        }
        __syncthreads();
        if (threadIdx.x == 0) extent[k] = make_uint2(sh_first, sh_last);
    }
}

}  // namespace

void rle_prefix_forward(hipStream_t s, const uint32_t* counts, const long long* run_offsets, long n_rle, uint32_t* pre_b, uint32_t* pre_o,
                        unsigned long long* totals, uint32_t* areas, uint2* extent)
{
    if (n_rle <= 0) return;
    hipLaunchKernelGGL(k_rle_prefix, dim3((unsigned)n_rle), dim3(256), 0, s, counts, run_offsets, n_rle, pre_b, pre_o, totals, areas, extent);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
