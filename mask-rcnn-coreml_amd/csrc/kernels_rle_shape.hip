// kernels_rle_shape.hip — measuring run-length masks (mrcnn_rle_measure, mrcnn_rle_convex_hull): moments, perimeter, convex hull and
// oriented box of every RLE of a flat set, from the runs, no plane and no scratch of an image's size.  The rules are shape_rule.h's;
// rle_shape_host.cpp is the definition these kernels must equal.  Everything is integer arithmetic, so sums may be taken in any order.
//
//   check      one thread per RLE: the lowest k whose total (rle_prefix_forward's) is not h*w; the caller reads it back before anything is written
//   moments    one block per RLE strides over the runs of ones.  A run is a head piece, a block of full columns and a tail piece, each a
//              closed form in its ends (shape_add_run): a full plane costs what one pixel costs.  Six int64 sums are reduced per block.
//   perimeter  one thread per VERTEX column X = 0 .. w of every RLE: one binary search per pixel column, then the merge of the pieces of
//              pixel columns X - 1 and X (touching pieces joined first; the column outside the plane is empty).  It adds the rows where the
//              two differ and 2 per piece of column X, and the total goes to the RLE's word by one 64-bit integer atomic per thread.
//   extremes   one thread per pixel column: the first set row t(x) and one past the last b(x), or the empty mark (-1, -1)
//   hull       one workgroup per RLE runs QuickHull on both chains at once, level by level as kernels_simplify.hip runs Douglas-Peucker:
//              every candidate that is neither kept nor dropped knows its chain segment (a, b); a round offers shape_key(c, position) to
//              the segment's slot (a 64-bit maximum: the largest c, the smallest position), reads the winner, and is dropped with the whole
//              segment (the winner's c is not positive), is the winner and kept, or takes the winner as its new a or b.  Up to
//              HULL_LDS_COLUMNS vertex columns the candidates' rows, segments and slots live in LDS, above in the RLE's carve of a
//              global scratch.  The slots have one side, so a round has three barriers; two sides would not fit 4096 columns.
//   scan       the hulls' counts -> hull_offsets; the caller reads the total back
//   write      one workgroup per RLE compacts the kept candidates into the ring and sums its shoelace terms
//   box        one workgroup per RLE, one thread per hull edge looping over the hull's vertices (shape_edge_box), then a block-wide
//              minimum by shape_box_before
// The number of launches depends on neither the number of RLEs nor the hulls' sizes.  No workgroup waits for another.
#include "kernels.h"
#include "scan_device.h"
#include "shape_rule.h"

namespace mrcnn {
namespace {

constexpr int TH = 256;
constexpr int HULL_TH = 512;

dim3 flat(long long n) { return dim3((unsigned)((n + TH - 1) / TH)); }
// one workgroup per RLE up to a grid that fills the device many times over; the rest by striding
dim3 per_rle(long long n) { return dim3((unsigned)(n < (1LL << 20) ? n : (1LL << 20))); }

__global__ __launch_bounds__(TH) void k_shape_check(ShapeSet S, unsigned long long* __restrict__ bad)
{
    const long long k = (long long)blockIdx.x * TH + threadIdx.x;
    if (k >= S.n) return;
    if (S.totals[k] != (unsigned long long)S.heights[k] * (unsigned long long)S.widths[k]) atomicMin(bad, (unsigned long long)k);
}

// ---- a pixel column's pieces ------------------------------------------------------------------------------------------------------------
// The maximal vertical pieces of pixel column x of one RLE in rising rows: one binary search in the prefix table, then a walk that ends
// at the column's end.  Zero-length runs neither start nor split a piece.
struct ShapeColumn {
    const uint32_t *B, *cnt;
    int nruns, j;
    uint32_t p0, p1;
    // valid = false: the column outside the plane, which has no piece
    __device__ ShapeColumn(const ShapeSet& S, int k, int x, bool valid)
    {
        const long long r0 = S.run_offsets[k];
        B = S.pre_b + r0; cnt = S.counts + r0;
        nruns = valid ? (int)(S.run_offsets[k + 1] - r0) : 0;
        const uint32_t h = (uint32_t)S.heights[k];
        p0 = (uint32_t)x * h; p1 = p0 + h;
        const uint32_t* b = B;
        j = nruns > 0 ? last_not_above(nruns, (long long)p0, [&](int i) { return (long long)b[i]; }) : 0;
    }
    __device__ bool next(int* a, int* b)
    {
        uint32_t lo = 0, hi = 0;
        bool found = false;
        for (; j < nruns && !found; ++j) {
            const uint32_t s = B[j];
            if (s >= p1) { j = nruns; return false; }
            const uint32_t n = cnt[j];
            if (!(j & 1) || !n || s + n <= p0) continue;
            lo = s > p0 ? s : p0; hi = s + n < p1 ? s + n : p1;
            found = true;
        }
        if (!found) return false;
        for (; j < nruns && hi < p1; ++j) {                      // the runs that touch the piece's end: zeros of length 0, then ones
            const uint32_t s = B[j];
            if (s > hi) break;
            const uint32_t n = cnt[j];
            if ((j & 1) && n) hi = s + n < p1 ? s + n : p1;
        }
        *a = (int)(lo - p0); *b = (int)(hi - p0);
        return true;
    }
};

// ---- moments ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(TH) void k_shape_moments(ShapeSet S, long long* __restrict__ measures)
{
    __shared__ long long part[TH / 64][6];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long k = blockIdx.x; k < S.n; k += gridDim.x) {
        const long long r0 = S.run_offsets[k], nruns = S.run_offsets[k + 1] - r0;
        const int h = S.heights[k];
        ShapeMoments m{0, 0, 0, 0, 0, 0};
        for (long long j = 2 * (long long)t + 1; j < nruns; j += 2 * TH) {       // the runs of ones
            const uint32_t n = S.counts[r0 + j];
            if (n) shape_add_run(m, S.pre_b[r0 + j], n, h);
        }
        const long long v[6] = {wave_sum(m.s1), wave_sum(m.sx), wave_sum(m.sy), wave_sum(m.sxx), wave_sum(m.sxy), wave_sum(m.syy)};
        if (lane == 0)
            for (int i = 0; i < 6; ++i) part[wave][i] = v[i];
        __syncthreads();
        if (t < 6) {
            long long sum = 0;
            for (int w = 0; w < TH / 64; ++w) sum += part[w][t];
            measures[SHAPE_MEASURE_WORDS * k + t] = sum;
        }
        __syncthreads();                                         // the next RLE reuses part
    }
}

// measures' perimeter words are zero when this starts
__global__ __launch_bounds__(TH) void k_shape_perimeter(ShapeSet S, long long* __restrict__ measures)
{
    const long long g = (long long)blockIdx.x * TH + threadIdx.x;
    if (g >= S.vcols) return;
    const int k = last_not_above(S.n, g, [&](int i) { return S.vcol0[i]; });
    const int X = (int)(g - S.vcol0[k]), w = S.widths[k];
    ShapeColumn A(S, k, X - 1, X >= 1), C(S, k, X, X < w);
    int a0 = 0, a1 = 0, c0 = 0, c1 = 0;
    bool ha = A.next(&a0, &a1), hc = C.next(&c0, &c1);
    long long len = 0, both = 0, pieces = 0;
    while (ha || hc) {                                           // (every round consumes a piece)
        if (ha && hc) {
            const int lo = max(a0, c0), hi = min(a1, c1);
            if (hi > lo) both += hi - lo;
        }
        if (ha && (!hc || a1 <= c1)) { len += a1 - a0; ha = A.next(&a0, &a1); }
        else { len += c1 - c0; ++pieces; hc = C.next(&c0, &c1); }
    }
    const long long sum = len - 2 * both + 2 * pieces;
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(measures + SHAPE_MEASURE_WORDS * (long long)k + 6), (unsigned long long)sum);
}

// ---- the hull ---------------------------------------------------------------------------------------------------------------------------
// ext[vcol0[k] + x] = (t, b) of pixel column x; the entry of vertex column w is the empty mark
__global__ __launch_bounds__(TH) void k_hull_extremes(ShapeSet S, int2* __restrict__ ext)
{
    const long long g = (long long)blockIdx.x * TH + threadIdx.x;
    if (g >= S.vcols) return;
    const int k = last_not_above(S.n, g, [&](int i) { return S.vcol0[i]; });
    const int x = (int)(g - S.vcol0[k]);
    ShapeColumn C(S, k, x, x < S.widths[k]);
    int a = 0, b = 0, t = -1, last = -1;
    while (C.next(&a, &b)) { t = t < 0 ? a : t; last = b; }
    ext[g] = make_int2(t, last);
}

// the row of the candidate at a position, -1 when the vertex column has none; e: the RLE's entries of ext
__device__ __forceinline__ int hull_candidate(const int2* __restrict__ e, int w, int pos)
{
    const int X = shape_position_x(pos, w);
    const int2 l = X > 0 ? e[X - 1] : make_int2(-1, -1), r = e[X];           // (e[w] is the empty mark)
    if (shape_position_top(pos, w)) return l.x < 0 ? r.x : (r.x < 0 ? l.x : min(l.x, r.x));
    return max(l.y, r.y);
}

// A ring's storage.  Both kinds answer y(pos); chain(i, &a, &b) / set_chain / retire for the candidate's own state, which only the
// thread that owns the candidate touches; offer / winner / clear for the slot of the segment that starts at a.  Positions are below
// 2 * 32768, so a segment's two ends are 16 bits each.
struct HullLds {
    unsigned long long* slot; int* y_; uint32_t* chain_;
    __device__ int y(int i) const { return y_[i]; }
    __device__ bool chain(int i, int* a, int* b) const
    {
        const uint32_t c = chain_[i];
        *a = (int)(c >> 16); *b = (int)(c & 0xffffu);
        return c != ~0u;
    }
    __device__ void set_chain(int i, int a, int b) { chain_[i] = ((uint32_t)a << 16) | (uint32_t)b; }
    __device__ void retire(int i) { chain_[i] = ~0u; }
    __device__ void offer(int a, unsigned long long key) { atomicMax(&slot[a], key); }
    __device__ unsigned long long winner(int a) const { return slot[a]; }
    __device__ void clear(int a) { slot[a] = 0; }
};
// The RLE's carve of the global scratch.  The slots are written and read with device-scope atomics, between the workgroup's barriers: a
// workgroup's own writes, seen by its other waves.  The rows come from ext, which an earlier launch wrote.
struct HullGlobal {
    unsigned long long* slot; const int2* e; uint32_t* chain_; int w;
    __device__ int y(int i) const { return hull_candidate(e, w, i); }
    __device__ bool chain(int i, int* a, int* b) const
    {
        const uint32_t c = chain_[i];
        *a = (int)(c >> 16); *b = (int)(c & 0xffffu);
        return c != ~0u;
    }
    __device__ void set_chain(int i, int a, int b) { chain_[i] = ((uint32_t)a << 16) | (uint32_t)b; }
    __device__ void retire(int i) { chain_[i] = ~0u; }
    __device__ void offer(int a, unsigned long long key) { atomicMax(&slot[a], key); }
    __device__ unsigned long long winner(int a) const { return __hip_atomic_load(&slot[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void clear(int a) { __hip_atomic_store(&slot[a], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// The rule on one non-empty RLE whose candidates span the vertex columns X0 .. X1; every thread of the block calls it.  keep: the m
// flags of the positions.  Returns how many candidates this thread kept.
template <class Ring>
__device__ int hull_ring(Ring R, int m, int w, int X0, int X1, uint8_t* __restrict__ keep)
{
    const int t = threadIdx.x;
    const int ta = X0, tb = X1, ba = 2 * w + 1 - X1, bb = 2 * w + 1 - X0;      // the ends of the top and of the bottom chain
    int kept = 0;
    for (int i = t; i < m; i += HULL_TH) {
        R.clear(i);
        const bool anchor = i == ta || i == tb || i == ba || i == bb;
        keep[i] = anchor ? 1 : 0;
        kept += anchor ? 1 : 0;
        if (anchor || R.y(i) < 0) R.retire(i);
        else if (i <= w) R.set_chain(i, ta, tb);
        else R.set_chain(i, ba, bb);
    }
    __syncthreads();
    // Every round either drops a whole segment or keeps one more candidate of it, so no segment is left after at most m rounds: the loop ends.
    for (;;) {
        bool live = false;
        for (int i = t; i < m; i += HULL_TH) {
            int a, b;
            if (!R.chain(i, &a, &b)) continue;
            live = true;
            R.offer(a, shape_key(shape_cross(shape_position_x(a, w), R.y(a), shape_position_x(b, w), R.y(b), shape_position_x(i, w), R.y(i)), i));
        }
        if (!__syncthreads_or(live ? 1 : 0)) break;              // (the whole block alike)
        for (int i = t; i < m; i += HULL_TH) {
            int a, b;
            if (!R.chain(i, &a, &b)) continue;
            const unsigned long long win = R.winner(a);
            const int k = simp_key_position(win);
            if (!shape_keeps(win)) R.retire(i);
            else if (i == k) { keep[i] = 1; ++kept; R.retire(i); }
            else if (i < k) R.set_chain(i, a, k);
            else R.set_chain(i, k, b);
        }
        __syncthreads();                                         // every winner is read
        for (int i = t; i < m; i += HULL_TH) {
            int a, b;
            if (R.chain(i, &a, &b)) R.clear(a);                  // the slots the next round offers to
        }
        __syncthreads();
    }
    return kept;
}

__global__ __launch_bounds__(HULL_TH) void k_hull_count(ShapeSet S, HullWork W, int lds_positions)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int first, last, total;
    const int t = threadIdx.x;
    HullLds L;
    L.slot = reinterpret_cast<unsigned long long*>(smem);
    L.y_ = reinterpret_cast<int*>(L.slot + lds_positions);
    L.chain_ = reinterpret_cast<uint32_t*>(L.y_ + lds_positions);
    for (long long k = blockIdx.x; k < S.n; k += gridDim.x) {
        const int w = S.widths[k], m = shape_positions(w);
        const long long v0 = S.vcol0[k];
        const int2* e = W.ext + v0;
        uint8_t* keep = W.keep + 2 * v0;
        if (t == 0) { first = w + 1; last = -1; total = 0; }
        __syncthreads();
        int lo = w + 1, hi = -1;                                 // the vertex columns with candidates
        for (int X = t; X <= w; X += HULL_TH)
            if (hull_candidate(e, w, X) >= 0) { lo = min(lo, X); hi = max(hi, X); }
        if (hi >= 0) { atomicMin(&first, lo); atomicMax(&last, hi); }
        __syncthreads();
        const int X0 = first, X1 = last;
        if (X1 < 0) {                                            // an empty mask has no hull (the whole block alike)
            for (int i = t; i < m; i += HULL_TH) keep[i] = 0;
            if (t == 0) W.count[k] = 0;
            __syncthreads();
            continue;
        }
        int kept;
        if (m <= lds_positions) {
            for (int i = t; i < m; i += HULL_TH) L.y_[i] = hull_candidate(e, w, i);
            __syncthreads();
            kept = hull_ring(L, m, w, X0, X1, keep);
        } else {
            if (!W.chain) continue;                              // (cannot be: the caller sized the scratch by the widest RLE)
            kept = hull_ring(HullGlobal{W.slot + 2 * v0, e, W.chain + 2 * v0, w}, m, w, X0, X1, keep);
        }
        atomicAdd(&total, kept);
        __syncthreads();
        if (t == 0) W.count[k] = (uint32_t)total;
        __syncthreads();                                         // the next RLE reuses first, last, total and the LDS
    }
}

// exclusive prefix of count[0 .. n) -> out[0 .. n]; one block
__global__ __launch_bounds__(1024) void k_hull_scan(const uint32_t* __restrict__ in, long long n, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(in, n, out, buf);
}

__global__ __launch_bounds__(TH) void k_hull_write(ShapeSet S, HullWork W, const long long* __restrict__ off, long long n_out, int32_t* xy,
                                                   long long* __restrict__ areas2)
{
    __shared__ int wave_n[4];
    __shared__ unsigned long long area;
    const int t = threadIdx.x;
    for (long long k = blockIdx.x; k < S.n; k += gridDim.x) {
        const int w = S.widths[k], m = shape_positions(w);
        const long long v0 = S.vcol0[k], o0 = off[k], cnt = off[k + 1] - o0;
        const int2* e = W.ext + v0;
        if (t == 0) area = 0;
        __syncthreads();
        long long run = 0;
        for (int base = 0; base < m; base += TH) {               // (the whole block alike)
            const int i = base + t;
            const bool kp = i < m && W.keep[2 * v0 + i] != 0;
            int n = 0;
            const long long at = run + compact_256(kp, wave_n, &n);
            if (kp && at < cnt && o0 + at < n_out) {             // (always, for the flags the count launch wrote)
                xy[2 * (o0 + at)] = shape_position_x(i, w);
                xy[2 * (o0 + at) + 1] = hull_candidate(e, w, i);
            }
            run += n;
            __syncthreads();
        }
        if (!areas2) continue;
        // twice the area: the shoelace terms of the ring as this workgroup has just written it
        const auto at = [&](long long j) { return (long long)__hip_atomic_load(&xy[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        long long sum = 0;
        if (o0 + cnt <= n_out)
            for (long long j = t; j < cnt; j += TH) {
                const long long p = 2 * (o0 + j), q = 2 * (o0 + (j + 1 < cnt ? j + 1 : 0));
                sum += at(p) * at(q + 1) - at(q) * at(p + 1);
            }
        atomicAdd(&area, (unsigned long long)sum);
        __syncthreads();
        if (t == 0) areas2[k] = (long long)area;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TH) void k_hull_box(long long n, const long long* __restrict__ off, const int32_t* __restrict__ xy, long long* __restrict__ obb)
{
    __shared__ ShapeScore score[TH];
    __shared__ int edge[TH];
    const int t = threadIdx.x;
    for (long long k = blockIdx.x; k < n; k += gridDim.x) {
        const long long o0 = off[k];
        const int m = (int)(off[k + 1] - o0);
        const int32_t* v = xy + 2 * o0;
        const auto X = [&](int i) { return v[2 * i]; };
        const auto Y = [&](int i) { return v[2 * i + 1]; };
        ShapeBox best{};
        ShapeScore bs{0, 0};
        int be = -1;
        for (int e = t; e < m; e += TH) {                        // rising e: a tie keeps the earlier edge
            const ShapeBox b = shape_edge_box(m, e, X, Y);
            const ShapeScore sc = shape_score(b);
            if (be >= 0 && !shape_box_before(sc, e, bs, be)) continue;
            best = b; bs = sc; be = e;
        }
        score[t] = bs; edge[t] = be;
        __syncthreads();
        for (int d = TH / 2; d >= 1; d >>= 1) {
            if (t < d && edge[t + d] >= 0 && (edge[t] < 0 || shape_box_before(score[t + d], edge[t + d], score[t], edge[t]))) {
                score[t] = score[t + d]; edge[t] = edge[t + d];
            }
            __syncthreads();
        }
        const int win = edge[0];
        long long* o = obb + SHAPE_OBB_WORDS * k;
        if (win < 0) {
            if (t < SHAPE_OBB_WORDS) o[t] = t == 0 ? -1 : 0;
        } else if (be == win) {
            o[0] = win; o[1] = best.dx; o[2] = best.dy; o[3] = best.dmin; o[4] = best.dmax; o[5] = best.cmin; o[6] = best.cmax; o[7] = 0;
        }
        __syncthreads();                                         // the next RLE reuses score and edge
    }
}

}  // namespace

void rle_shape_check_forward(hipStream_t s, const ShapeSet& S, unsigned long long* bad)
{
    HIP_CHECK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), s));
    if (S.n <= 0) return;
    hipLaunchKernelGGL(k_shape_check, flat(S.n), dim3(TH), 0, s, S, bad);
    HIP_CHECK(hipGetLastError());
}

void rle_shape_measure_forward(hipStream_t s, const ShapeSet& S, long long* measures)
{
    if (S.n <= 0) return;
    HIP_CHECK(hipMemsetAsync(measures, 0, (size_t)S.n * SHAPE_MEASURE_WORDS * sizeof(long long), s));
    hipLaunchKernelGGL(k_shape_moments, per_rle(S.n), dim3(TH), 0, s, S, measures);
    hipLaunchKernelGGL(k_shape_perimeter, flat(S.vcols), dim3(TH), 0, s, S, measures);
    HIP_CHECK(hipGetLastError());
}

void rle_hull_count_forward(hipStream_t s, const ShapeSet& S, const HullWork& W, int max_w, long long* hull_offsets)
{
    if (S.n <= 0) return;
    hipLaunchKernelGGL(k_hull_extremes, flat(S.vcols), dim3(TH), 0, s, S, W.ext);
    const int cols = max_w + 1 < HULL_LDS_COLUMNS ? max_w + 1 : HULL_LDS_COLUMNS;
    const size_t bytes = (size_t)cols * HULL_LDS_BYTES_PER_COLUMN;
    HIP_CHECK(hipFuncSetAttribute((const void*)k_hull_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(k_hull_count, per_rle(S.n), dim3(HULL_TH), bytes, s, S, W, 2 * cols);
    hipLaunchKernelGGL(k_hull_scan, dim3(1), dim3(1024), 0, s, W.count, (long long)S.n, reinterpret_cast<unsigned long long*>(hull_offsets));
    HIP_CHECK(hipGetLastError());
}

void rle_hull_write_forward(hipStream_t s, const ShapeSet& S, const HullWork& W, const long long* hull_offsets, long long n_out, int32_t* xy,
                            long long* areas2, long long* obb)
{
    if (S.n <= 0) return;
    hipLaunchKernelGGL(k_hull_write, per_rle(S.n), dim3(TH), 0, s, S, W, hull_offsets, n_out, xy, areas2);
    if (obb) hipLaunchKernelGGL(k_hull_box, per_rle(S.n), dim3(TH), 0, s, (long long)S.n, hull_offsets, xy, obb);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
