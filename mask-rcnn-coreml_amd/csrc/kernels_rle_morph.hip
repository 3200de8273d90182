// kernels_rle_morph.hip — morphology with a square structuring element on a set of run-length masks (mrcnn_rle_morph): RLE in, RLE out,
// no dense byte plane and no scratch of an image's size.  The rule is morph_rule.h's; rle_morph_host.cpp is the definition.
//
// The square of radius r is a vertical line of 2r + 1 followed by a horizontal one.  The vertical half is free in the run domain: the
// set pixels of a column are intervals, and the line shrinks or grows each interval (morph_interval).  The horizontal half runs on
// bits: the result of the vertical half is written as a packed BIT BOX per RLE — the box the result lies in (morph_work_box), 32 rows
// per uint32 word, the words of one word row side by side: word (j, c) of a box of bw columns at j * bw + c — and an output word is
// the AND (erosion) or OR (dilation) of the 2r + 1 words around it in its word row.
//   k_morph_box        one block per RLE: the tight box of its set pixels from the runs, and the lowest RLE with a wrong total
//   (the host reads the boxes back once and lays out the bit boxes, the columns and the tiles: the scratch follows the masks)
//   k_morph_vertical   one thread per column of a box: one binary search in the prefix table, then the column's runs; it writes the
//                      words of its own column, so nothing is atomic.  BOUNDARY writes the mask's own bits beside them.
//   k_morph_horizontal one block per tile of one word row: C + 2r words staged in LDS and combined by doubling — after step k entry i
//                      holds the words i .. i + 2^k - 1, and two overlapping entries of the last step cover 2r + 1 — then P & ~E for
//                      BOUNDARY.  Lanes read and write neighbouring LDS words at every step: no bank is hit twice.
//   k_morph_count / k_morph_write   the encoder of rle_device.h on the bits, with poly_offsets_forward's scan between them.
// Seven launches whatever the number of RLEs.
#include "kernels.h"
#include "morph_rule.h"
#include "rle_device.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

__global__ __launch_bounds__(256) void k_morph_box(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ pre_b,
                                                   const long long* __restrict__ run_offsets, const int32_t* __restrict__ heights,
                                                   const int32_t* __restrict__ widths, const unsigned long long* __restrict__ totals,
                                                   const uint2* __restrict__ extent, MorphBox* __restrict__ tight, unsigned long long* __restrict__ bad)
{
    const long k = blockIdx.x;
    const int h = heights[k], w = widths[k];
    const uint2 e = extent[k];
    const bool wrong = totals[k] != (unsigned long long)h * (unsigned long long)w;
    if (wrong || e.x > e.y) {                                // (uniform) refused, or no set pixel: the empty box
        if (threadIdx.x == 0) {
            if (wrong) atomicMin(bad, (unsigned long long)k);
            tight[k] = MorphBox{0, 0, 0, 0};
        }
        return;
    }
    __shared__ int s_lo, s_hi;
    if (threadIdx.x == 0) { s_lo = h; s_hi = -1; }
    __syncthreads();
    int lo = h, hi = -1;
    const long long r0 = run_offsets[k], r1 = run_offsets[k + 1];
    for (long long j = r0 + 1 + 2 * (long long)threadIdx.x; j < r1; j += 512) {      // the runs of ones
        const uint32_t c = counts[j];
        if (!c) continue;
        const uint32_t first = pre_b[j], last = first + c - 1, cf = first / (uint32_t)h, cl = last / (uint32_t)h;
        if (cf != cl) { lo = 0; hi = h - 1; }                // over a column's end: it leaves at the bottom row and enters at the top
        else { lo = min(lo, (int)(first - cf * (uint32_t)h)); hi = max(hi, (int)(last - cf * (uint32_t)h)); }
    }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    if (threadIdx.x == 0) tight[k] = MorphBox{s_lo, (int)(e.x / (uint32_t)h), s_hi + 1, (int)(e.y / (uint32_t)h) + 1};
}

// The words of one column of a bit box, written once each from the top: add() takes bit intervals in rising order.
struct MorphColumn {
    uint32_t* col; long long stride; int words;
    int j = 0; uint32_t acc = 0;
    __device__ __forceinline__ void flush_to(int wj) { for (; j < wj; ++j) { col[j * stride] = acc; acc = 0; } }
    __device__ __forceinline__ void add(int a, int b)        // bits [a, b), 0 <= a < b <= 32 * words (held to that: nothing is written outside the column)
    {
        a = max(a, 0); b = min(b, 32 * words);
        while (a < b) {
            const int wj = a >> 5, top = min(b, (wj + 1) << 5), n = top - a;
            flush_to(wj);
            acc |= (n == 32 ? 0xffffffffu : (1u << n) - 1u) << (a & 31);
            a = top;
        }
    }
    __device__ __forceinline__ void finish() { flush_to(words); }
};

__global__ __launch_bounds__(256) void k_morph_vertical(const MorphJob job)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= job.cols) return;
    const int k = last_not_above(job.n, g, [&](int i) { return job.rec[i].col0; });
    const MorphRec q = job.rec[k];
    const int bw = q.work.x2 - q.work.x1, c = (int)(g - q.col0), x = q.work.x1 + c;
    const bool grows = morph_grows(job.op), keep = job.op == MRCNN_MORPH_BOUNDARY;
    MorphColumn V{job.va + q.word0 + c, bw, q.words}, P{job.vb + q.word0 + c, bw, q.words};
    auto emit = [&](int a, int b) {                          // a joined interval of this column
        int oa, ob;
        if (keep) P.add(a - q.work.y1, b - q.work.y1);
        if (morph_interval(a, b, q.r, q.h, grows, &oa, &ob)) V.add(oa - q.work.y1, ob - q.work.y1);
    };
    if (x >= q.tight.x1 && x < q.tight.x2) {                 // (a column the box only grew into has no run of ones)
        const uint32_t p0 = (uint32_t)x * (uint32_t)q.h, p1 = p0 + (uint32_t)q.h;
        const uint32_t* B = job.pre_b + q.r0;
        const uint32_t* cnt = job.counts + q.r0;
        int pa = -1, pb = -1;                                // the interval that may still be joined
        for (int j = last_not_above(q.nruns, (long long)p0, [&](int i) { return (long long)B[i]; }); j < q.nruns; ++j) {
            const uint32_t s = B[j];
            if (s >= p1) break;
            const uint32_t n = cnt[j];
            if (!(j & 1) || !n) continue;
            const int a = (int)(max(s, p0) - p0), b = (int)(min(s + n, p1) - p0);
            if (pa >= 0 && morph_joins(pb, a, q.r, grows)) { pb = b; continue; }
            if (pa >= 0) emit(pa, pb);
            pa = a; pb = b;
        }
        if (pa >= 0) emit(pa, pb);
    }
    V.finish();
    if (keep) P.finish();
}

__global__ __launch_bounds__(256) void k_morph_horizontal(const MorphJob job)
{
    __shared__ uint32_t buf[2][MORPH_TILE];                  // 32 KB
    const long long t = blockIdx.x;
    const int k = last_not_above(job.n, t, [&](int i) { return job.rec[i].tile0; });
    const MorphRec q = job.rec[k];
    const int bw = q.work.x2 - q.work.x1, C = MORPH_TILE - 2 * q.r, chunks = (bw + C - 1) / C;
    const int local = (int)(t - q.tile0), j = local / chunks, c0 = (local % chunks) * C;
    const int cw = min(C, bw - c0), staged = cw + 2 * q.r;   // staged <= MORPH_TILE
    const bool grows = morph_grows(job.op);
    const long long row = q.word0 + (long long)j * bw;
    for (int i = threadIdx.x; i < staged; i += 256) {        // entry i: column c0 - r + i of the box; outside the box is 0
        const int col = c0 - q.r + i;
        buf[0][i] = col >= 0 && col < bw ? job.va[row + col] : 0u;
    }
    __syncthreads();
    const int win = 2 * q.r + 1, K = 31 - __clz(win);
    int cur = 0;
    for (int s = 0; s < K; ++s) {                            // (uniform)
        const int step = 1 << s;
        for (int i = threadIdx.x; i < staged; i += 256) {
            uint32_t v = buf[cur][i];
            if (i + step < staged) v = grows ? v | buf[cur][i + step] : v & buf[cur][i + step];
            buf[cur ^ 1][i] = v;
        }
        cur ^= 1;
        __syncthreads();
    }
    const int second = win - (1 << K);                       // entries c and c + second cover c .. c + 2r
    for (int c = threadIdx.x; c < cw; c += 256) {
        const uint32_t a = buf[cur][c], b = buf[cur][c + second];
        const uint32_t e = grows ? a | b : a & b;
        uint32_t* o = job.vb + row + c0 + c;
        *o = job.op == MRCNN_MORPH_BOUNDARY ? *o & ~e : e;
    }
}

// the result's bit of pixel (x, y); y = -1 / y = h as rle_device.h's rle_bit takes them
struct MorphBit {
    const uint32_t* bits; int4 bx; int bw, h;
    __device__ __forceinline__ bool operator()(int x, int y) const
    {
        if (y < 0) { --x; y = h - 1; } else if (y >= h) { ++x; y = 0; }
        if (x < bx.y || x >= bx.w || y < bx.x || y >= bx.z) return false;
        const int b = y - bx.x;
        return (bits[(long long)(b >> 5) * bw + (x - bx.y)] >> (b & 31)) & 1u;
    }
};

__device__ __forceinline__ RleWalk morph_walk(const MorphRec& q)
{
    RleWalk k;
    k.bx = make_int4(q.work.y1, q.work.x1, q.work.y2, q.work.x2); k.m = nullptr; k.S = 0; k.h = q.h; k.w = q.w; k.thr = 0.0f;
    rle_walk_box(k);
    return k;
}

__global__ __launch_bounds__(1024) void k_morph_count(const MorphJob job, RleSeg* __restrict__ segs, uint32_t* __restrict__ nruns,
                                                      uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes)
{
    const MorphRec q = job.rec[blockIdx.x];
    const RleWalk k = morph_walk(q);
    rle_count_plane(k, MorphBit{job.vb + q.word0, k.bx, q.work.x2 - q.work.x1, q.h}, (size_t)blockIdx.x, segs, nruns, areas, bboxes);
}

__global__ __launch_bounds__(1024) void k_morph_write(const MorphJob job, const RleSeg* __restrict__ segs, const long long* __restrict__ run_offsets,
                                                      uint32_t* __restrict__ counts)
{
    const MorphRec q = job.rec[blockIdx.x];
    const RleWalk k = morph_walk(q);
    rle_write_plane(k, MorphBit{job.vb + q.word0, k.bx, q.work.x2 - q.work.x1, q.h}, (size_t)blockIdx.x, segs, run_offsets[blockIdx.x],
                    run_offsets[blockIdx.x + 1], counts);
}

}  // namespace

void rle_morph_boxes_forward(hipStream_t s, const uint32_t* counts, const uint32_t* pre_b, const long long* run_offsets, const int32_t* heights,
                             const int32_t* widths, const unsigned long long* totals, const uint2* extent, long n, MorphBox* tight,
                             unsigned long long* bad)
{
    HIP_CHECK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
    if (n <= 0) return;
    hipLaunchKernelGGL(k_morph_box, dim3((unsigned)n), dim3(256), 0, s, counts, pre_b, run_offsets, heights, widths, totals, extent, tight, bad);
    HIP_CHECK(hipGetLastError());
}

void rle_morph_forward(hipStream_t s, const MorphJob& job)
{
    if (job.cols > 0) {
        hipLaunchKernelGGL(k_morph_vertical, dim3((unsigned)((job.cols + 255) / 256)), dim3(256), 0, s, job);
        HIP_CHECK(hipGetLastError());
    }
    if (job.tiles > 0) {
        hipLaunchKernelGGL(k_morph_horizontal, dim3((unsigned)job.tiles), dim3(256), 0, s, job);
        HIP_CHECK(hipGetLastError());
    }
}

void rle_morph_count_forward(hipStream_t s, const MorphJob& job, RleSeg* segs, uint32_t* nruns, long long* run_offsets, uint32_t* areas, int32_t* bboxes)
{
    if (job.n > 0) {
        hipLaunchKernelGGL(k_morph_count, dim3((unsigned)job.n), dim3(64 * RLE_SEGS), 0, s, job, segs, nruns, areas, bboxes);
        HIP_CHECK(hipGetLastError());
    }
    poly_offsets_forward(s, nruns, job.n, run_offsets);
}

void rle_morph_write_forward(hipStream_t s, const MorphJob& job, const RleSeg* segs, const long long* run_offsets, uint32_t* counts)
{
    if (job.n <= 0) return;
    hipLaunchKernelGGL(k_morph_write, dim3((unsigned)job.n), dim3(64 * RLE_SEGS), 0, s, job, segs, run_offsets, counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
