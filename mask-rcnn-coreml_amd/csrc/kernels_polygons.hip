// kernels_polygons.hip — run-length masks to polygon rings (mrcnn_rle_to_polygons).  The kernels work on runs and corners, never on a
// decoded plane; polygons_host.cpp, which walks pixels, is the definition they must equal, and polygon_rule.h is what the two share.
//
//   count   one thread per vertex column X of an RLE: a binary search in the prefix table finds the runs of pixel columns X-1 and X, a
//           merge walk visits the rows where either changes, polygon_rule.h says how many corners the vertex there has
//   scan    the corners of the set back to back in (RLE, X, Y) order; the caller reads the total and the largest RLE back
//   corners the same walk writes them
//   trace   a corner's vertical piece ends at its neighbour in that order (corner ^ 1: every column holds an even number); its horizontal
//           piece ends at its neighbour in the row order, which a bitonic sort of (Y, X) finds.  The walk's successor is one of the two.
//           Pointer jumping then gives every corner the smallest corner of its cycle and the steps to it.  One block in LDS per RLE of
//           at most POLYGON_LDS_CORNERS corners; the others in global memory, one launch per sort step and per jumping round.
//   write   scans over the ring leaders number the rings and place their vertices; every corner is written once, at its final place
//
// Every loop is bounded before it starts: by the runs of two columns, by log2 of a size the host knows, or by a fixed stride.  The only
// atomics are integer minimum, maximum and sum, whose results do not depend on their order.
// Algorithmic bytes per corner, LDS path: 4 written + 4 read (the word), 12 written (succ, lead, dist), 8 + 16 (heads, scans), 8 (xy).
#include "kernels.h"
#include "polygon_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

constexpr uint32_t NO_CORNER = 0xffffffffu;

// ---- units ---------------------------------------------------------------------------------------------------------------
struct Unit { long long k, r0, r1; int h, w, X; };

__device__ inline Unit unit_of(const PolygonSet& set, long long u)
{
    const PolygonImage* tab = set.tab;
    const int b = last_not_above(set.n_images, u, [&](int i) { return tab[i].unit0; });
    const long long r = u - tab[b].unit0;
    const int cols = tab[b].w + 1;
    Unit t;
    t.h = tab[b].h; t.w = tab[b].w;
    t.k = (long long)b * set.slots + r / cols;
    t.X = (int)(r % cols);
    t.r0 = set.run_offsets[t.k]; t.r1 = set.run_offsets[t.k + 1];
    return t;
}

__device__ inline long long first_unit(const PolygonSet& set, long long k)
{
    const int b = (int)(k / set.slots);
    return set.tab[b].unit0 + (k % set.slots) * (long long)(set.tab[b].w + 1);
}

// One pixel column of an RLE that sums to its plane, read top to bottom: `state` holds for the rows up to `end` (a position, exclusive).
// A column outside the plane is unset from top to bottom.
struct Column {
    const uint32_t* B;
    long long j, r0, r1;
    uint32_t total, lo, hi, end;
    int state;

    __device__ uint32_t run_end(long long i) const { return i + 1 < r1 ? B[i + 1] : total; }
    __device__ void open(const uint32_t* pre_b, long long r0_, long long r1_, uint32_t total_, int col, int h, bool inside)
    {
        B = pre_b; r0 = r0_; r1 = r1_; total = total_;
        if (!inside) { lo = 0; hi = end = (uint32_t)h; state = 0; j = r1; return; }
        lo = (uint32_t)col * (uint32_t)h; hi = lo + (uint32_t)h;
        const uint32_t* first = pre_b + r0;
        const int i = last_not_above((int)(r1 - r0), (long long)lo, [&](int q) { return (long long)first[q]; });   // (B[r0] = 0 <= lo)
        j = r0 + i;                                              // the last run that starts at or before lo: the one that holds it
        state = i & 1;
        end = min(run_end(j), hi);
    }
    // the run that holds position `end` (end < hi <= total, so there is one; at most r1 - j steps)
    __device__ void next()
    {
        do ++j; while (j + 1 < r1 && run_end(j) <= end);
        state = (int)((j - r0) & 1);
        end = min(run_end(j), hi);
    }
    __device__ int row() const { return (int)(end - lo); }
};

// calls emit(i, Y, corner) for the corners of vertex column X from the top, i = 0, 1, ...; returns their number
template <class Emit>
__device__ inline int walk_vertex_column(const uint32_t* __restrict__ pre_b, const Unit& t, Emit&& emit)
{
    const uint32_t total = (uint32_t)t.h * (uint32_t)t.w;
    Column left, right;
    left.open(pre_b, t.r0, t.r1, total, t.X - 1, t.h, t.X >= 1);
    right.open(pre_b, t.r0, t.r1, total, t.X, t.h, t.X < t.w);
    PolyNbhd nb{0, 0, left.state, right.state};
    int y = 0, n = 0;
    for (;;) {                                                   // (one round per row where a column changes: at most the runs of both)
        PolyCorner c[2];
        const int m = poly_corners(nb, c);
        for (int i = 0; i < m; ++i) emit(n++, y, c[i]);
        if (y >= t.h) break;
        const int yl = left.row(), yr = right.row();
        const int ny = min(yl, yr);
        nb.tl = left.state; nb.tr = right.state;
        if (ny >= t.h) { nb.bl = 0; nb.br = 0; }
        else {
            if (yl == ny) left.next();
            if (yr == ny) right.next();
            nb.bl = left.state; nb.br = right.state;
        }
        y = ny;
    }
    return n;
}

__device__ inline bool sums_to_plane(const PolygonSet& set, const Unit& t)
{
    return set.totals[t.k] == (unsigned long long)t.h * (unsigned long long)t.w;
}

__global__ __launch_bounds__(256) void k_polygon_check(PolygonSet set, long long n, unsigned long long* __restrict__ summary)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const PolygonImage g = set.tab[k / set.slots];
    if (set.totals[k] != (unsigned long long)g.h * (unsigned long long)g.w) atomicMin(&summary[0], (unsigned long long)k);
}

__global__ __launch_bounds__(256) void k_polygon_count(PolygonSet set)
{
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= set.units) return;
    const Unit t = unit_of(set, u);
    set.unit_cnt[u] = sums_to_plane(set, t) ? (uint32_t)walk_vertex_column(set.pre_b, t, [](int, int, const PolyCorner&) {}) : 0u;
}

// exclusive prefix of in[0 .. n) -> out[0 .. n]; one block
__global__ __launch_bounds__(1024) void k_polygon_scan(const uint32_t* __restrict__ in, long long n, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(in, n, out, buf);
}

__global__ __launch_bounds__(256) void k_polygon_ranges(PolygonSet set, long long n, unsigned long long* __restrict__ summary)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > n) return;
    const unsigned long long c0 = set.unit_start[k < n ? first_unit(set, k) : set.units];
    set.corner0[k] = (long long)c0;
    if (k == n) { summary[1] = c0; return; }
    const unsigned long long c1 = set.unit_start[k + 1 < n ? first_unit(set, k + 1) : set.units];
    atomicMax(&summary[2], c1 - c0);
}

__global__ __launch_bounds__(256) void k_polygon_corners(PolygonSet set, long long n_corners, uint32_t* __restrict__ corner)
{
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= set.units) return;
    const unsigned long long at = set.unit_start[u];
    const uint32_t cnt = set.unit_cnt[u];
    if (cnt == 0 || at + cnt > (unsigned long long)n_corners) return;
    const Unit t = unit_of(set, u);
    walk_vertex_column(set.pre_b, t, [&](int i, int y, const PolyCorner& c) {
        if ((uint32_t)i < cnt) corner[at + i] = poly_pack(t.X, y, c);
    });
}

// ---- an RLE in LDS ------------------------------------------------------------------------------------------------------
constexpr int LDS_N = POLYGON_LDS_CORNERS;
constexpr int LDS_PER_THREAD = LDS_N / 256;
static_assert(LDS_N >= 512 && (LDS_N & (LDS_N - 1)) == 0, "MRCNN_POLYGON_LDS_CORNERS must be a power of two, two per thread at least");

__device__ inline int ceil_log2(unsigned long long m)
{
    int r = 0;
    while (r < 63 && (1ull << r) < m) ++r;
    return r;
}

// The step of the pointer jumping, round r: `mine` and `theirs` are (smallest corner << 32 | steps to it) over the 2^r corners from
// here and over the 2^r after them.  Equal minima are one corner met again after a lap: the first meeting counts.
__device__ inline unsigned long long jump(unsigned long long mine, unsigned long long theirs, int r)
{
    return (theirs >> 32) < (mine >> 32) ? theirs + (1ull << r) : mine;
}

__global__ __launch_bounds__(256) void k_polygon_trace_lds(const long long* __restrict__ corner0, const uint32_t* __restrict__ corner,
                                                            uint32_t* __restrict__ succ, uint32_t* __restrict__ lead, uint32_t* __restrict__ dist)
{
    const long long c0 = corner0[blockIdx.x];
    const long long mm = corner0[blockIdx.x + 1] - c0;
    if (mm <= 0 || mm > LDS_N) return;                           // (the whole block alike)
    const int m = (int)mm, t0 = threadIdx.x;
    __shared__ unsigned long long keys[LDS_N], md[LDS_N];
    __shared__ uint32_t nx[LDS_N], out_succ[LDS_N];
    int P = 2;
    while (P < m) P <<= 1;                                       // <= LDS_N
    for (int i = t0; i < P; i += 256)
        keys[i] = i < m ? ((unsigned long long)poly_packed_row_key(corner[c0 + i]) << 32) | (unsigned)i : ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = t0; t < P / 2; t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const unsigned long long a = keys[i], b = keys[p];
                if ((a > b) == ((i & kk) == 0)) { keys[i] = b; keys[p] = a; }
            }
            __syncthreads();
        }
    // the row order: places 2q and 2q + 1 hold the two ends of a horizontal piece
    for (int p = t0; p < m; p += 256) {
        const uint32_t i = (uint32_t)keys[p], q = (uint32_t)keys[p ^ 1];
        uint32_t s = poly_packed_leaves_vertically(corner[c0 + i]) ? (i ^ 1u) : q;            // (c0 is even: every column holds an even number)
        if (s >= (uint32_t)m) s = i;                             // (cannot be: m is even and the padding sorts behind every corner)
        out_succ[i] = s; nx[i] = s;
        md[i] = (unsigned long long)i << 32;
    }
    __syncthreads();
    const int rounds = ceil_log2((unsigned long long)m);
    for (int r = 0; r < rounds; ++r) {
        uint32_t nn[LDS_PER_THREAD];
        unsigned long long v[LDS_PER_THREAD];
#pragma unroll
        for (int e = 0; e < LDS_PER_THREAD; ++e) {
            const int i = t0 + 256 * e;
            if (i < m) { const uint32_t a = nx[i]; nn[e] = nx[a]; v[e] = jump(md[i], md[a], r); }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < LDS_PER_THREAD; ++e) {
            const int i = t0 + 256 * e;
            if (i < m) { nx[i] = nn[e]; md[i] = v[e]; }
        }
        __syncthreads();
    }
    for (int i = t0; i < m; i += 256) {
        succ[c0 + i] = (uint32_t)c0 + out_succ[i];
        lead[c0 + i] = (uint32_t)c0 + (uint32_t)(md[i] >> 32);
        dist[c0 + i] = (uint32_t)md[i];
    }
}

// ---- the larger RLEs in global memory ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_polygon_big_sizes(const long long* __restrict__ corner0, long long n, uint32_t* __restrict__ pad_size)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const long long m = corner0[k + 1] - corner0[k];
    pad_size[k] = m > LDS_N ? 1u << ceil_log2((unsigned long long)m) : 0u;        // (m < 2^31)
}

// place g of the padded slices -> its RLE and its place in the slice; false behind the last slice
struct BigPlace { long long k, c0; unsigned long long slice; uint32_t l, size, m; };
__device__ inline bool big_place(const unsigned long long* __restrict__ pad_start, const long long* __restrict__ corner0, long long n, unsigned long long g,
                                 BigPlace* p)
{
    if (g >= pad_start[n]) return false;
    const int k = last_not_above((int)n, (long long)g, [&](int i) { return (long long)pad_start[i]; });    // (the last of equal starts: the one with a slice)
    p->k = k; p->c0 = corner0[k]; p->slice = pad_start[k];
    p->l = (uint32_t)(g - pad_start[k]); p->size = (uint32_t)(pad_start[k + 1] - pad_start[k]); p->m = (uint32_t)(corner0[k + 1] - corner0[k]);
    return true;
}

__global__ __launch_bounds__(256) void k_polygon_big_fill(const unsigned long long* __restrict__ pad_start, const long long* __restrict__ corner0, long long n,
                                                           const uint32_t* __restrict__ corner, unsigned long long* __restrict__ sort)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    BigPlace p;
    if (!big_place(pad_start, corner0, n, g, &p)) return;
    sort[g] = p.l < p.m ? ((unsigned long long)poly_packed_row_key(corner[p.c0 + p.l]) << 32) | p.l : ~0ull;
}

__global__ __launch_bounds__(256) void k_polygon_big_sort(const unsigned long long* __restrict__ pad_start, const long long* __restrict__ corner0, long long n,
                                                           uint32_t kk, uint32_t j, unsigned long long* __restrict__ sort)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    BigPlace p;
    if (!big_place(pad_start, corner0, n, g, &p)) return;
    if (kk > p.size || (p.l & j)) return;                        // this slice is sorted already / the pair's upper place
    const unsigned long long a = sort[g], b = sort[g + j];       // (l + j < size: j < kk <= size and bit j of l is clear)
    if ((a > b) == ((p.l & kk) == 0)) { sort[g] = b; sort[g + j] = a; }
}

__global__ __launch_bounds__(256) void k_polygon_big_succ(const unsigned long long* __restrict__ pad_start, const long long* __restrict__ corner0, long long n,
                                                           const uint32_t* __restrict__ corner, const unsigned long long* __restrict__ sort,
                                                           uint32_t* __restrict__ succ, uint32_t* __restrict__ next, unsigned long long* __restrict__ md)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    BigPlace p;
    if (!big_place(pad_start, corner0, n, g, &p) || p.l >= p.m) return;
    const uint32_t i = (uint32_t)sort[g], q = (uint32_t)sort[p.slice + (p.l ^ 1u)];
    if (i >= p.m || q >= p.m) return;                            // (cannot be: m is even and the padding sorts behind every corner)
    const uint32_t c = (uint32_t)p.c0 + i;
    const uint32_t s = poly_packed_leaves_vertically(corner[c]) ? (c ^ 1u) : (uint32_t)p.c0 + q;
    succ[c] = s; next[c] = s;
    md[c] = (unsigned long long)c << 32;
}

// one round for every corner of the larger RLEs (the others hold NO_CORNER on both sides and stay so)
__global__ __launch_bounds__(256) void k_polygon_big_jump(long long n_corners, int r, const uint32_t* __restrict__ next_in,
                                                           const unsigned long long* __restrict__ md_in, uint32_t* __restrict__ next_out,
                                                           unsigned long long* __restrict__ md_out)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const uint32_t a = next_in[c];
    if (a == NO_CORNER || a >= (unsigned long long)n_corners) return;
    const uint32_t b = next_in[a];
    if (b == NO_CORNER) return;
    next_out[c] = b;
    md_out[c] = jump(md_in[c], md_in[a], r);
}

__global__ __launch_bounds__(256) void k_polygon_big_done(long long n_corners, const uint32_t* __restrict__ next, const unsigned long long* __restrict__ md,
                                                           uint32_t* __restrict__ lead, uint32_t* __restrict__ dist)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners || next[c] == NO_CORNER) return;
    lead[c] = (uint32_t)(md[c] >> 32);
    dist[c] = (uint32_t)md[c];
}

// ---- rings ----------------------------------------------------------------------------------------------------------------
// a ring's smallest corner knows the ring's length: its successor is that many steps, less one, away from it
__global__ __launch_bounds__(256) void k_polygon_heads(long long n_corners, const uint32_t* __restrict__ succ, const uint32_t* __restrict__ lead,
                                                        const uint32_t* __restrict__ dist, uint32_t* __restrict__ head, uint32_t* __restrict__ len)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const bool first = lead[c] == (uint32_t)c;
    const uint32_t s = succ[c];
    head[c] = first ? 1u : 0u;
    len[c] = first && s < (unsigned long long)n_corners ? dist[s] + 1u : 0u;
}

__global__ __launch_bounds__(256) void k_polygon_rle_rings(const long long* __restrict__ corner0, long long n, const unsigned long long* __restrict__ ring_id,
                                                            long long* __restrict__ rle_rings)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k <= n) rle_rings[k] = (long long)ring_id[corner0[k]];
}

__global__ __launch_bounds__(256) void k_polygon_write(PolygonWork w, long long n_corners, long long n_rings, long long* __restrict__ ring_offsets,
                                                        unsigned long long* __restrict__ ring_areas, int32_t* __restrict__ xy)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const uint32_t first = w.lead[c], word = w.corner[c];
    if (first >= (unsigned long long)n_corners) return;
    const long long ring = (long long)w.ring_id[first];
    const uint32_t d = w.dist[c], length = w.len[first];
    const long long at = (long long)w.vertex0[first] + (d == 0 ? 0u : length - d);
    if (ring >= n_rings || at >= n_corners || d > length) return;          // (cannot be for a permutation)
    const int x = poly_packed_x(word), y = poly_packed_y(word);
    xy[2 * at] = x; xy[2 * at + 1] = y;
    if (c == first) ring_offsets[ring] = (long long)w.vertex0[first];
    if (c == 0) ring_offsets[n_rings] = n_corners;
    // the area is the sum of x * dy over the vertical pieces: the shoelace sum with its horizontal terms, which are zero, left out
    if (ring_areas && poly_packed_leaves_vertically(word)) {
        const uint32_t s = w.succ[c];
        if (s < (unsigned long long)n_corners)
            atomicAdd(&ring_areas[ring], (unsigned long long)((long long)x * (long long)(poly_packed_y(w.corner[s]) - y)));
    }
}

dim3 flat(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

void polygons_count_forward(hipStream_t s, const PolygonSet& set, unsigned long long* summary)
{
    const long long n = (long long)set.n_images * set.slots;
    HIP_CHECK(hipMemsetAsync(summary, 0xff, sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(summary + 1, 0, 2 * sizeof(unsigned long long), s));
    if (n <= 0 || set.units <= 0) return;
    hipLaunchKernelGGL(k_polygon_check, flat(n), dim3(256), 0, s, set, n, summary);
    hipLaunchKernelGGL(k_polygon_count, flat(set.units), dim3(256), 0, s, set);
    hipLaunchKernelGGL(k_polygon_scan, dim3(1), dim3(1024), 0, s, set.unit_cnt, set.units, set.unit_start);
    hipLaunchKernelGGL(k_polygon_ranges, flat(n + 1), dim3(256), 0, s, set, n, summary);
    HIP_CHECK(hipGetLastError());
}

void polygons_trace_forward(hipStream_t s, const PolygonSet& set, const PolygonWork& w, long long n_corners, long long most, long long* rle_rings)
{
    const long long n = (long long)set.n_images * set.slots;
    if (n <= 0 || n_corners <= 0) return;
    hipLaunchKernelGGL(k_polygon_corners, flat(set.units), dim3(256), 0, s, set, n_corners, w.corner);
    hipLaunchKernelGGL(k_polygon_trace_lds, dim3((unsigned)n), dim3(256), 0, s, set.corner0, w.corner, w.succ, w.lead, w.dist);
    if (most > POLYGON_LDS_CORNERS) {
        const int rounds = [&] { int r = 0; while ((1ll << r) < most) ++r; return r; }();
        const long long padded = 2 * n_corners;                  // bounds the sum of the padded sizes
        HIP_CHECK(hipMemsetAsync(w.next_a, 0xff, (size_t)n_corners * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(w.next_b, 0xff, (size_t)n_corners * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_polygon_big_sizes, flat(n), dim3(256), 0, s, set.corner0, n, w.pad_size);
        hipLaunchKernelGGL(k_polygon_scan, dim3(1), dim3(1024), 0, s, w.pad_size, n, w.pad_start);
        hipLaunchKernelGGL(k_polygon_big_fill, flat(padded), dim3(256), 0, s, w.pad_start, set.corner0, n, w.corner, w.sort);
        for (int a = 1; a <= rounds; ++a)
            for (int b = a - 1; b >= 0; --b)
                hipLaunchKernelGGL(k_polygon_big_sort, flat(padded), dim3(256), 0, s, w.pad_start, set.corner0, n, 1u << a, 1u << b, w.sort);
        hipLaunchKernelGGL(k_polygon_big_succ, flat(padded), dim3(256), 0, s, w.pad_start, set.corner0, n, w.corner, w.sort, w.succ, w.next_a, w.md_a);
        uint32_t *na = w.next_a, *nb = w.next_b;
        unsigned long long *ma = w.md_a, *mb = w.md_b;
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(k_polygon_big_jump, flat(n_corners), dim3(256), 0, s, n_corners, r, na, ma, nb, mb);
            std::swap(na, nb); std::swap(ma, mb);
        }
        hipLaunchKernelGGL(k_polygon_big_done, flat(n_corners), dim3(256), 0, s, n_corners, na, ma, w.lead, w.dist);
    }
    hipLaunchKernelGGL(k_polygon_heads, flat(n_corners), dim3(256), 0, s, n_corners, w.succ, w.lead, w.dist, w.head, w.len);
    hipLaunchKernelGGL(k_polygon_scan, dim3(1), dim3(1024), 0, s, w.head, n_corners, w.ring_id);
    hipLaunchKernelGGL(k_polygon_scan, dim3(1), dim3(1024), 0, s, w.len, n_corners, w.vertex0);
    hipLaunchKernelGGL(k_polygon_rle_rings, flat(n + 1), dim3(256), 0, s, set.corner0, n, w.ring_id, rle_rings);
    HIP_CHECK(hipGetLastError());
}

void polygons_write_forward(hipStream_t s, const PolygonWork& w, long long n_corners, long long n_rings, long long* ring_offsets, long long* ring_areas,
                            int32_t* xy)
{
    if (n_corners <= 0) return;
    if (ring_areas) HIP_CHECK(hipMemsetAsync(ring_areas, 0, (size_t)n_rings * sizeof(long long), s));
    hipLaunchKernelGGL(k_polygon_write, flat(n_corners), dim3(256), 0, s, w, n_corners, n_rings, ring_offsets,
                       reinterpret_cast<unsigned long long*>(ring_areas), xy);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
