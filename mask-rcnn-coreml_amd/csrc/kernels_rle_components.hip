// kernels_rle_components.hip — connected components of a set of run-length masks (mrcnn_rle_components, mrcnn_rle_components_select):
// runs in, measures or runs out, no dense plane.  The rule is components_rule.h's; rle_components_host.cpp is the definition.
//
// The nodes are PIECES: a run of the labelled value cut at the ends of its pixel columns, touching pieces of one column joined first
// (zero-length runs of the other value may lie between two runs).  A piece is rows [a, b) of one column; its index order is the
// column-major order of its first pixel.
//   k_cc_check    one thread per RLE: the lowest RLE whose total is not its plane's
//   k_cc_count    one thread per run: the pieces the run owns (those that START in it); k_cc_scan gives every run its first piece
//   k_cc_pieces   one thread per piece: a binary search finds its run, then the piece's start and end POSITION (x*h + y) and its RLE
//   k_cc_link     one thread per piece: one binary search in the RLE's piece ends finds the first piece of column x + 1 that can meet
//                 it, then a walk; every meeting pair is united in the parent array: find both roots, hang the larger root under the
//                 smaller with an integer compare-and-swap, retry from the value read.  Only roots are ever hooked and a parent only
//                 falls, so the root of a component is its lowest piece whatever the order of execution; finds halve their path with
//                 atomicMin (an ancestor stays an ancestor).  No thread waits for another.
//   k_cc_flatten  the root of every piece into a second array (nothing is written to the parents any more), root flags
//   k_cc_scan     root flags -> component numbers: the rule's order for free
//   k_cc_number   the number of every piece's component, the components' RLEs, comp_offsets
//   k_cc_measure  integer atomics into the component's area, box and flag (a wave whose pieces are of one component adds once);
//   k_cc_final    the measures as the entry writes them
// The selection writes RLEs from a SEQUENCE of pieces cut into GROUPS, one group per output RLE — MERGE: the pieces as they lie, one
// group per RLE; SPLIT: the pieces sorted by (component, piece) with a bitonic network on unique 64-bit keys, in LDS below SORT_CHUNK
// entries apart and grid-wide above, one group per kept component:
//   k_cc_bcount   a kept piece starts a run of the labelled value unless the piece before it in the sequence is kept, of its group
//                 and ends where this one starts — what joins a run across a column end — and ends one likewise; the plane's own two
//                 ends are no boundaries.  k_cc_scan; k_cc_groups: runs per group; poly_offsets_forward: out_run_offsets
//   k_cc_bwrite   the boundaries' positions;  k_cc_runs: one thread per output run, the difference of two boundaries, and the ones
//                 runs' areas and boxes by integer atomics;  k_cc_gfinal: areas and boxes as the entry writes them
// The number of launches depends on neither the number of RLEs nor the number of components; SPLIT's sort adds launches with the
// square of the logarithm of the number of pieces.
#include <limits.h>

#include <algorithm>

#include "kernels.h"
#include "components_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

using u64 = unsigned long long;

__device__ __forceinline__ int rle_of_run(const CompSet& S, long long j)
{
    return last_not_above(S.n, j, [&](int i) { return S.run_offsets[i]; });
}

// Run j as a source of pieces: false when it is not of the labelled value, empty, or of an RLE that does not sum to its plane.
// [s, e): its positions; first_col: the first column in which a piece starts in it; cols: how many do.
__device__ inline bool run_pieces(const CompSet& S, long long j, int* k_out, uint32_t* s_out, uint32_t* e_out, uint32_t* first_col, uint32_t* cols)
{
    const int k = rle_of_run(S, j);
    const long long r0 = S.run_offsets[k];
    const uint32_t h = (uint32_t)S.heights[k];
    if ((int)((j - r0) & 1) != S.of) return false;
    const uint32_t n = S.counts[j];
    if (!n || S.totals[k] != (u64)h * (u64)S.widths[k]) return false;
    const uint32_t s = S.pre_b[j], e = s + n, cf = s / h, cl = (e - 1) / h;
    long long i = j - 1;
    while (i >= r0 && S.counts[i] == 0) --i;                 // the run before it that holds a pixel: of the same value, they touch
    const bool joined = i >= r0 && ((j - i) & 1) == 0 && s != cf * h;
    *k_out = k; *s_out = s; *e_out = e;
    *first_col = cf + (joined ? 1u : 0u);
    *cols = cl - cf + 1 - (joined ? 1u : 0u);
    return true;
}

__global__ __launch_bounds__(256) void k_cc_check(const CompSet S, u64* __restrict__ bad)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= S.n) return;
    if (S.totals[k] != (u64)S.heights[k] * (u64)S.widths[k]) atomicMin(bad, (u64)k);
}

__global__ __launch_bounds__(256) void k_cc_count(const CompSet S, long long runs, uint32_t* __restrict__ run_cnt)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= runs) return;
    int k; uint32_t s, e, c0, cols;
    run_cnt[j] = run_pieces(S, S.run_offsets[0] + j, &k, &s, &e, &c0, &cols) ? cols : 0u;
}

// exclusive prefix of in[0 .. n) -> out[0 .. n]; one block
__global__ __launch_bounds__(1024) void k_cc_scan(const uint32_t* __restrict__ in, long long n, u64* __restrict__ out)
{
    __shared__ u64 buf[2][1024];
    scan_array(in, n, out, buf);
}

__global__ __launch_bounds__(256) void k_cc_pieces(const CompSet S, long long runs, const u64* __restrict__ run_start, CompPieces P)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P.n) return;
    const long long jr = last_not_above((int)runs, p, [&](int i) { return (long long)run_start[i]; });
    const long long j = S.run_offsets[0] + jr;
    int k; uint32_t s, e, c0, cols;
    uint32_t a = 0, b = 0;
    if (run_pieces(S, j, &k, &s, &e, &c0, &cols)) {          // (always: a run without pieces owns no index)
        const uint32_t h = (uint32_t)S.heights[k], col = c0 + (uint32_t)(p - (long long)run_start[jr]), end = (col + 1) * h;
        a = max(s, col * h); b = min(e, end);
        if (b == e && b < end) {                             // the run ends inside the column: runs that touch it belong to the piece
            const long long r1 = S.run_offsets[k + 1];
            for (long long i = j + 1; i < r1 && b < end; ++i) {
                const uint32_t n = S.counts[i];
                if (!n) continue;
                if ((i - j) & 1) break;                      // a pixel of the other value ends it
                b = min(b + n, end);
            }
        }
    } else k = 0;
    P.pa[p] = a; P.pb[p] = b; P.rle[p] = k; P.parent[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void k_cc_piece0(const CompSet S, const u64* __restrict__ run_start, long long* __restrict__ piece0)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > S.n) return;
    piece0[k] = (long long)run_start[S.run_offsets[k] - S.run_offsets[0]];
}

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// the root of x; every node passed is hung under its grandparent (atomicMin: a parent only falls, and to an ancestor)
__device__ inline uint32_t cc_find(uint32_t* parent, uint32_t x)
{
    uint32_t p = cc_load(parent + x);
    while (p != x) {                                         // (a chain falls strictly: at most x rounds)
        const uint32_t g = cc_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p; p = g;
    }
    return x;
}

__device__ inline void cc_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    a = cc_find(parent, a); b = cc_find(parent, b);
    while (a != b) {                                         // (every retry continues from a smaller node: it ends)
        if (a < b) { const uint32_t t = a; a = b; b = t; }   // a is the larger
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return;                                // a was a root and hangs under b now
        a = cc_find(parent, old);                            // somebody hooked a first: go on from where it points
        b = cc_find(parent, b);
    }
}

__global__ __launch_bounds__(256) void k_cc_link(const CompSet S, const CompPieces P, const long long* __restrict__ piece0, int conn)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P.n) return;
    const int k = P.rle[p];
    const uint32_t h = (uint32_t)S.heights[k], w = (uint32_t)S.widths[k];
    const uint32_t pa = P.pa[p], x = pa / h;
    if (x + 1 >= w) return;
    const int a = (int)(pa - x * h), b = (int)(P.pb[p] - x * h), d = conn == 8 ? 1 : 0;
    const uint32_t next = (x + 1) * h;
    // the first piece of column x + 1 whose end lies past row a (a - 1 for 8): every piece of a column up to x ends at `next` or before
    const uint32_t past = next + (uint32_t)max(a - d, 0);
    long long lo = piece0[k], hi = piece0[k + 1];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (P.pb[mid] > past) hi = mid; else lo = mid + 1;
    }
    const long long end = piece0[k + 1];
    for (long long q = lo; q < end; ++q) {
        const uint32_t qa = P.pa[q];
        if (qa >= next + h) break;
        const int c = (int)(qa - next), e = (int)(P.pb[q] - next);
        if (c >= b + d) break;
        if (components_meet(a, b, c, e, conn)) cc_unite(P.parent, (uint32_t)p, (uint32_t)q);
    }
}

__global__ __launch_bounds__(256) void k_cc_flatten(const CompPieces P, uint32_t* __restrict__ is_root)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P.n) return;
    uint32_t x = (uint32_t)p, q = P.parent[x];
    while (q != x) { x = q; q = P.parent[x]; }
    P.root[p] = x;
    is_root[p] = x == (uint32_t)p;
}

// comp[p]: the number of p's component in the whole set; comp_rle[c]: its RLE; comp_offsets[k]
__global__ __launch_bounds__(256) void k_cc_number(const CompPieces P, const u64* __restrict__ comp_start, const long long* __restrict__ piece0, int n,
                                                   int32_t* __restrict__ comp_rle, long long* __restrict__ comp_offsets)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p <= n) comp_offsets[p] = (long long)comp_start[piece0[p]];
    if (p >= P.n) return;
    const uint32_t r = P.root[p];
    const uint32_t c = (uint32_t)comp_start[r];
    P.comp[p] = c;
    if (r == (uint32_t)p) comp_rle[c] = P.rle[p];
}

__global__ __launch_bounds__(256) void k_cc_measure(const CompSet S, const CompPieces P, CompAcc acc)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < P.n;
    uint32_t c = 0xffffffffu, area = 0;
    int x = 0, y1 = INT_MAX, y2 = 0, flag = 0;
    if (live) {
        const int k = P.rle[p];
        const uint32_t h = (uint32_t)S.heights[k], pa = P.pa[p];
        c = P.comp[p]; x = (int)(pa / h);
        y1 = (int)(pa - (uint32_t)x * h); y2 = (int)(P.pb[p] - (uint32_t)x * h);
        area = (uint32_t)(y2 - y1);
        flag = components_on_border(x, y1, y2, (int)h, S.widths[k]);
    }
    int x1 = live ? x : INT_MAX, x2 = live ? x : 0;
    const uint32_t c0 = __shfl(c, 0, 64);
    const bool one = __all(c == c0 || !live) && c0 != 0xffffffffu;      // (uniform) the wave's pieces are of one component: lane 0 is live
    if (one) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            area += __shfl_down(area, s, 64);
            x1 = min(x1, __shfl_down(x1, s, 64)); x2 = max(x2, __shfl_down(x2, s, 64));
            y1 = min(y1, __shfl_down(y1, s, 64)); y2 = max(y2, __shfl_down(y2, s, 64));
            flag |= __shfl_down(flag, s, 64);
        }
        if ((threadIdx.x & 63) != 0) return;
    } else if (!live) return;
    atomicAdd(acc.area + c, area);
    atomicMin(acc.x1 + c, x1); atomicMax(acc.x2 + c, x2);
    atomicMin(acc.y1 + c, y1); atomicMax(acc.y2 + c, y2);
    if (flag) atomicOr(acc.flag + c, 1u);
}

__global__ __launch_bounds__(256) void k_cc_final(const CompAcc acc, long long n_comps, uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes,
                                                  uint8_t* __restrict__ flags)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_comps) return;
    areas[c] = acc.area[c];
    bboxes[4 * c + 0] = acc.x1[c]; bboxes[4 * c + 1] = acc.y1[c];
    bboxes[4 * c + 2] = acc.x2[c] - acc.x1[c] + 1; bboxes[4 * c + 3] = acc.y2[c] - acc.y1[c];
    flags[c] = (uint8_t)acc.flag[c];
}

// ---- SPLIT's order: the pieces sorted by (component, piece) -----------------------------------------------------------------------
constexpr int SORT_CHUNK = 2048;                             // keys a block sorts in LDS (16 KB)

__global__ __launch_bounds__(256) void k_cc_sort_fill(const CompPieces P, long long padded, u64* __restrict__ keys)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;
    keys[i] = i < P.n ? ((u64)P.comp[i] << 32 | (u64)i) : ~0ull;
}

// the steps (k, j) of the network with j < m, for k = k_from, 2 k_from, .. k_to: a block holds m neighbouring keys (m <= SORT_CHUNK)
__global__ __launch_bounds__(1024) void k_cc_sort_lds(u64* __restrict__ keys, int m, long long k_from, long long k_to)
{
    __shared__ u64 sh[SORT_CHUNK];
    const long long base = (long long)blockIdx.x * m;
    for (int i = threadIdx.x; i < m; i += 1024) sh[i] = keys[base + i];
    __syncthreads();
    for (long long k = k_from; k <= k_to; k <<= 1)
        for (int j = (int)min(k >> 1, (long long)(m >> 1)); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < m / 2; t += 1024) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const bool up = ((base + i) & k) == 0;
                const u64 a = sh[i], b = sh[l];
                if ((a > b) == up) { sh[i] = b; sh[l] = a; }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < m; i += 1024) keys[base + i] = sh[i];
}

__global__ __launch_bounds__(256) void k_cc_sort_step(u64* __restrict__ keys, long long pairs, long long k, long long j)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs) return;
    const long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
    const bool up = (i & k) == 0;
    const u64 a = keys[i], b = keys[l];
    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
}

// order[i] = the piece at place i of the sorted sequence; comp_first[c] = the place of component c's first piece (comp_first[C] = n)
__global__ __launch_bounds__(256) void k_cc_sort_done(const u64* __restrict__ keys, long long n, long long n_comps, uint32_t* __restrict__ order,
                                                      long long* __restrict__ comp_first)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) comp_first[n_comps] = n;
    if (i >= n) return;
    const u64 key = keys[i];
    order[i] = (uint32_t)key;
    if (i == 0 || (keys[i - 1] >> 32) != (key >> 32)) comp_first[key >> 32] = i;
}

// ---- the writer ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_keep_flags(const uint8_t* __restrict__ keep, long long n_comps, uint32_t* __restrict__ flag)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < n_comps) flag[c] = keep[c] != 0;
}

// SPLIT's groups: kept component c is output RLE out_index[c]
__global__ __launch_bounds__(256) void k_cc_split_groups(const uint8_t* __restrict__ keep, const u64* __restrict__ out_index, long long n_comps,
                                                         const long long* __restrict__ comp_first, const int32_t* __restrict__ comp_rle, CompGroups G,
                                                         long long* __restrict__ out_parent)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_comps || !keep[c]) return;
    const long long g = (long long)out_index[c];
    G.begin[g] = comp_first[c]; G.end[g] = comp_first[c + 1]; G.rle[g] = comp_rle[c];
    out_parent[g] = comp_rle[c];
}

__global__ __launch_bounds__(256) void k_cc_merge_groups(const long long* __restrict__ piece0, long long n, CompGroups G, long long* __restrict__ out_parent)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    G.begin[k] = piece0[k]; G.end[k] = piece0[k + 1]; G.rle[k] = (int32_t)k;
    if (out_parent) out_parent[k] = k;
}

// The sequence the writer walks.  place i holds piece order[i] (MERGE: i itself); its group is its RLE (MERGE) or its component (SPLIT):
// two neighbours of the sequence are of one group when those agree.
struct CompSeq {
    CompPieces P; const uint32_t* order; const uint8_t* keep; int split;
    __device__ __forceinline__ uint32_t piece(long long i) const { return order ? order[i] : (uint32_t)i; }
    __device__ __forceinline__ bool kept(uint32_t q) const { return keep[P.comp[q]] != 0; }
    __device__ __forceinline__ bool together(uint32_t q, uint32_t r) const { return split ? P.comp[q] == P.comp[r] : P.rle[q] == P.rle[r]; }
    // the boundaries place i gives: bit 0 its start, bit 1 its end
    __device__ inline int boundaries(long long i, const CompSet& S, uint32_t* pa, uint32_t* pb) const
    {
        const uint32_t q = piece(i);
        if (!kept(q)) return 0;
        const uint32_t a = P.pa[q], b = P.pb[q];
        *pa = a; *pb = b;
        bool starts = a != 0, ends = b != (uint32_t)S.heights[P.rle[q]] * (uint32_t)S.widths[P.rle[q]];      // the plane's own ends are none
        if (starts && i > 0) {
            const uint32_t r = piece(i - 1);
            if (P.pb[r] == a && together(q, r) && kept(r)) starts = false;
        }
        if (ends && i + 1 < P.n) {
            const uint32_t r = piece(i + 1);
            if (P.pa[r] == b && together(q, r) && kept(r)) ends = false;
        }
        return (starts ? 1 : 0) | (ends ? 2 : 0);
    }
};

__global__ __launch_bounds__(256) void k_cc_bcount(const CompSet S, const CompSeq Q, uint32_t* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.P.n) return;
    uint32_t a, b;
    cnt[i] = (uint32_t)__popc(Q.boundaries(i, S, &a, &b));
}

__global__ __launch_bounds__(256) void k_cc_bwrite(const CompSet S, const CompSeq Q, const u64* __restrict__ bpos, uint32_t* __restrict__ bnd)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.P.n) return;
    uint32_t a, b;
    const int f = Q.boundaries(i, S, &a, &b);
    u64 at = bpos[i];
    if (f & 1) bnd[at++] = a;
    if (f & 2) bnd[at] = b;
}

// runs per group: the boundaries, the run that closes the plane, and a leading empty run of zeros when the plane starts with a one
__global__ __launch_bounds__(256) void k_cc_groups(const CompSet S, const CompSeq Q, CompGroups G, const u64* __restrict__ bpos)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= G.n) return;
    const long long i0 = G.begin[g], i1 = G.end[g];
    bool first = false;                                      // pixel 0 is of the labelled value in the result
    if (i0 < i1) {
        const uint32_t q = Q.piece(i0);
        first = Q.P.pa[q] == 0 && Q.kept(q);
    }
    const uint32_t lead = (first ? S.of : !S.of) ? 1u : 0u;
    G.lead[g] = lead;
    G.nruns[g] = lead + (uint32_t)(bpos[i1] - bpos[i0]) + 1u;
    G.area[g] = 0; G.x1[g] = INT_MAX; G.y1[g] = INT_MAX; G.x2[g] = -1; G.y2[g] = -1;
}

__global__ __launch_bounds__(256) void k_cc_runs(const CompSet S, const CompGroups G, const u64* __restrict__ bpos, const uint32_t* __restrict__ bnd,
                                                 const long long* __restrict__ out_off, long long total, uint32_t* __restrict__ counts, int measure)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= total) return;
    const int g = last_not_above((int)G.n, r, [&](int i) { return out_off[i]; });       // (every group has a run: the offsets rise strictly)
    const int i = (int)(r - out_off[g]), lead = (int)G.lead[g], k = G.rle[g];
    const uint32_t h = (uint32_t)S.heights[k], hw = h * (uint32_t)S.widths[k];
    uint32_t lo = 0, hi = 0;
    if (i >= lead) {
        const long long b0 = (long long)bpos[G.begin[g]], nb = (long long)G.nruns[g] - lead - 1, bi = i - lead;
        lo = bi == 0 ? 0u : bnd[b0 + bi - 1];
        hi = bi == nb ? hw : bnd[b0 + bi];
    }
    if (counts) counts[r] = hi - lo;
    if (!measure || !(i & 1) || hi == lo) return;
    const int xa = (int)(lo / h), xb = (int)((hi - 1) / h);
    atomicAdd(G.area + g, hi - lo);
    atomicMin(G.x1 + g, xa); atomicMax(G.x2 + g, xb);
    atomicMin(G.y1 + g, xa != xb ? 0 : (int)(lo - (uint32_t)xa * h));
    atomicMax(G.y2 + g, xa != xb ? (int)h - 1 : (int)(hi - 1 - (uint32_t)xa * h));
}

__global__ __launch_bounds__(256) void k_cc_gfinal(const CompGroups G, uint32_t* __restrict__ areas, int32_t* __restrict__ bboxes)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= G.n) return;
    const bool any = G.area[g] > 0;
    if (areas) areas[g] = G.area[g];
    if (!bboxes) return;
    bboxes[4 * g + 0] = any ? G.x1[g] : 0; bboxes[4 * g + 1] = any ? G.y1[g] : 0;
    bboxes[4 * g + 2] = any ? G.x2[g] - G.x1[g] + 1 : 0; bboxes[4 * g + 3] = any ? G.y2[g] - G.y1[g] + 1 : 0;
}

inline dim3 flat(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

void rle_components_count_forward(hipStream_t s, const CompSet& S, long long runs, uint32_t* run_cnt, unsigned long long* run_start, unsigned long long* bad)
{
    HIP_CHECK(hipMemsetAsync(bad, 0xff, sizeof(u64), s));
    if (S.n > 0) hipLaunchKernelGGL(k_cc_check, flat(S.n), dim3(256), 0, s, S, bad);
    if (runs > 0) hipLaunchKernelGGL(k_cc_count, flat(runs), dim3(256), 0, s, S, runs, run_cnt);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, run_cnt, runs, run_start);
    HIP_CHECK(hipGetLastError());
}

void rle_components_label_forward(hipStream_t s, const CompSet& S, long long runs, const unsigned long long* run_start, const CompPieces& P,
                                  long long* piece0, uint32_t* is_root, unsigned long long* comp_start, int32_t* comp_rle, long long* comp_offsets)
{
    hipLaunchKernelGGL(k_cc_piece0, flat(S.n + 1), dim3(256), 0, s, S, run_start, piece0);
    if (P.n > 0) {
        hipLaunchKernelGGL(k_cc_pieces, flat(P.n), dim3(256), 0, s, S, runs, run_start, P);
        hipLaunchKernelGGL(k_cc_link, flat(P.n), dim3(256), 0, s, S, P, piece0, components_connectivity(S.connectivity, S.of));
        hipLaunchKernelGGL(k_cc_flatten, flat(P.n), dim3(256), 0, s, P, is_root);
    }
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, is_root, P.n, comp_start);
    hipLaunchKernelGGL(k_cc_number, flat(std::max(P.n, (long long)S.n + 1)), dim3(256), 0, s, P, comp_start, piece0, S.n, comp_rle, comp_offsets);
    HIP_CHECK(hipGetLastError());
}

void rle_components_measure_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompAcc& acc, long long n_comps, uint32_t* areas,
                                    int32_t* bboxes, uint8_t* flags)
{
    if (n_comps <= 0) return;
    const size_t C = (size_t)n_comps;
    HIP_CHECK(hipMemsetAsync(acc.area, 0, C * 4, s));
    HIP_CHECK(hipMemsetAsync(acc.flag, 0, C * 4, s));
    HIP_CHECK(hipMemsetAsync(acc.x1, 0x7f, C * 4, s));
    HIP_CHECK(hipMemsetAsync(acc.y1, 0x7f, C * 4, s));
    HIP_CHECK(hipMemsetAsync(acc.x2, 0, C * 4, s));
    HIP_CHECK(hipMemsetAsync(acc.y2, 0, C * 4, s));
    hipLaunchKernelGGL(k_cc_measure, flat(P.n), dim3(256), 0, s, S, P, acc);
    hipLaunchKernelGGL(k_cc_final, flat(n_comps), dim3(256), 0, s, acc, n_comps, areas, bboxes, flags);
    HIP_CHECK(hipGetLastError());
}

long long rle_components_sort_padded(long long n_pieces)
{
    long long p = 2;
    while (p < n_pieces) p <<= 1;
    return p;
}

void rle_components_sort_forward(hipStream_t s, const CompPieces& P, long long n_comps, unsigned long long* keys, uint32_t* order, long long* comp_first)
{
    const long long padded = rle_components_sort_padded(P.n);
    const int m = (int)std::min(padded, (long long)SORT_CHUNK);
    const unsigned blocks = (unsigned)(padded / m);
    hipLaunchKernelGGL(k_cc_sort_fill, flat(padded), dim3(256), 0, s, P, padded, keys);
    hipLaunchKernelGGL(k_cc_sort_lds, dim3(blocks), dim3(1024), 0, s, keys, m, 2LL, (long long)m);
    for (long long k = 2LL * m; k <= padded; k <<= 1) {
        for (long long j = k >> 1; j >= m; j >>= 1) hipLaunchKernelGGL(k_cc_sort_step, flat(padded / 2), dim3(256), 0, s, keys, padded / 2, k, j);
        hipLaunchKernelGGL(k_cc_sort_lds, dim3(blocks), dim3(1024), 0, s, keys, m, k, k);
    }
    hipLaunchKernelGGL(k_cc_sort_done, flat(std::max(P.n, 1LL)), dim3(256), 0, s, keys, P.n, n_comps, order, comp_first);
    HIP_CHECK(hipGetLastError());
}

void rle_components_keep_forward(hipStream_t s, const uint8_t* keep, long long n_comps, uint32_t* flag, unsigned long long* out_index)
{
    if (n_comps > 0) hipLaunchKernelGGL(k_cc_keep_flags, flat(n_comps), dim3(256), 0, s, keep, n_comps, flag);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, flag, n_comps, out_index);
    HIP_CHECK(hipGetLastError());
}

void rle_components_groups_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompSelect& q, const long long* piece0,
                                   const int32_t* comp_rle, const CompGroups& G, uint32_t* bcnt, unsigned long long* bpos, long long* out_parent,
                                   long long* out_run_offsets)
{
    const CompSeq Q{P, q.order, q.keep, q.order != nullptr};
    if (G.n > 0) {
        if (q.order) hipLaunchKernelGGL(k_cc_split_groups, flat(q.n_comps), dim3(256), 0, s, q.keep, q.out_index, q.n_comps, q.comp_first, comp_rle, G, out_parent);
        else hipLaunchKernelGGL(k_cc_merge_groups, flat(G.n), dim3(256), 0, s, piece0, G.n, G, out_parent);
    }
    if (P.n > 0) hipLaunchKernelGGL(k_cc_bcount, flat(P.n), dim3(256), 0, s, S, Q, bcnt);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, bcnt, P.n, bpos);
    if (G.n > 0) hipLaunchKernelGGL(k_cc_groups, flat(G.n), dim3(256), 0, s, S, Q, G, bpos);
    HIP_CHECK(hipGetLastError());
    poly_offsets_forward(s, G.nruns, (long)G.n, out_run_offsets);
    if (G.n <= 0) HIP_CHECK(hipMemsetAsync(out_run_offsets, 0, sizeof(long long), s));
}

void rle_components_write_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompSelect& q, const CompGroups& G,
                                  const unsigned long long* bpos, uint32_t* bnd, const long long* out_run_offsets, long long total_runs, uint32_t* counts,
                                  uint32_t* areas, int32_t* bboxes)
{
    if (G.n <= 0) return;
    const CompSeq Q{P, q.order, q.keep, q.order != nullptr};
    const int measure = areas || bboxes;
    if (P.n > 0) hipLaunchKernelGGL(k_cc_bwrite, flat(P.n), dim3(256), 0, s, S, Q, bpos, bnd);
    hipLaunchKernelGGL(k_cc_runs, flat(total_runs), dim3(256), 0, s, S, G, bpos, bnd, out_run_offsets, total_runs, counts, measure);
    if (measure) hipLaunchKernelGGL(k_cc_gfinal, flat(G.n), dim3(256), 0, s, G, areas, bboxes);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
