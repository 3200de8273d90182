// scan_device.h — the block-wide searches and scans more than one kernel file needs: the search that maps a unit of a ragged batch to its
// image and the one-block prefix sums of the encoders' scan and pack launches (kernels_jpeg_enc.hip, kernels_png.hip), and the
// compaction of the drawing kernels' cull passes (kernels_render.hip, kernels_rle_draw.hip).  Device code only; every loop is bounded
// by an argument.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mrcnn {

// the last entry of first[0 .. n) that is <= g (first[0] <= g)
template <class Get>
__device__ inline int last_not_above(int n, long long g, Get first)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                   // (at most log2(n) + 1 rounds)
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Compaction over the 256 threads of a block; every thread calls it.  Returns this thread's position in the list of the threads whose
// `keep` is set, in thread order, and *n = the list's length.  wave_n: four ints of LDS, free again after the caller's next barrier
// (one barrier inside).
__device__ __forceinline__ int compact_256(bool keep, int* wave_n, int* n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = wave_n[k];
        before += k < wave ? c : 0;
        all += c;
    }
    *n = all;
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// inclusive sum over the 1024 threads of a block; every thread calls it.  buf is free again when it returns.
__device__ inline unsigned long long scan_1024(unsigned long long mine, unsigned long long (*buf)[1024], unsigned long long* total)
{
    const int t = threadIdx.x;
    int cur = 0;
    buf[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        buf[cur ^ 1][t] = buf[cur][t] + (t >= d ? buf[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long mine_incl = buf[cur][t];
    *total = buf[cur][1023];
    __syncthreads();
    return mine_incl;
}

// exclusive scan of in[0 .. n) -> out[0 .. n], out[n] = the sum; one block of 1024.  A round covers 4096 entries: a thread sums four
// neighbours itself, the block scans the 1024 sums, the thread finishes its four
__device__ inline void scan_array(const uint32_t* __restrict__ in, long long n, unsigned long long* __restrict__ out, unsigned long long (*buf)[1024])
{
    const int t = threadIdx.x;
    unsigned long long carry = 0, total;
    for (long long base = 0; base < n; base += 4096) {
        const long long i0 = base + 4 * t;
        unsigned long long v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
        const unsigned long long mine = v[0] + v[1] + v[2] + v[3];
        unsigned long long run = carry + scan_1024(mine, buf, &total) - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) out[i0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (t == 0) out[n] = carry;
    __threadfence();
    __syncthreads();                                    // the block reads out[] next
}

}  // namespace mrcnn
