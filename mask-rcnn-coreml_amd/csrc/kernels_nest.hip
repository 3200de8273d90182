// kernels_nest.hip — polygon rings nested into outlines and their holes (mrcnn_polygons_nest).  nest_host.cpp, which loops over rings and
// edges one by one, is the definition these kernels must equal, and nest_rule.h is what the two share.  Every quantity is an integer and
// every choice a strict order, so the split of the loops over workgroups, waves and lanes cannot change a bit.
//
//   check    rle_rings per RLE and ring_offsets per ring -> summary[0], summary[1]
//   measure  one wave per ring, the lanes striding over its vertices: |area2|, the bounding box, the owning RLE (a binary search in
//            rle_rings) and the coordinates' range -> summary[2].  The caller reads the summary back before anything is written.
//   parent   one workgroup per target ring r.  Its four waves stride over the candidate rings q of r's RLE; a candidate that does not
//            outrank r, cannot beat the wave's best so far, or whose bounding box does not hold probe(r) strictly inside is skipped —
//            a closed ring crosses the line y = Y0 + 1/2 an even number of times and, outside the box, all or none of them left of the
//            probe, so the cull cannot change a parity.  The lanes stride over q's edges (two coalesced int32 pairs each), the parity is
//            one ballot, every wave keeps its closest candidate and thread 0 picks the parent from the four in LDS.
//   depth    one thread per ring walks to its root (at most the RLE's rings: a forest), marks shells and counts the holes of each shell
//   sizes    scan of the shell flags -> a shell's polygon; 1 + holes per shell, scan -> where a polygon starts in ring_order
//   place    one wave per ring: a shell writes poly_rings and itself; a hole ranks itself among its siblings by counting the rings of
//            its RLE before it that have the same parent (ballots over coalesced reads of parent) and takes that place behind its shell
//   rles     rle_polys[k] = the polygons before RLE k's first ring
//
// Eight launches and two one-block scans, whatever the rings and the RLEs.  The walk is the one loop whose length depends on the data: a
// chain of depth D has D rings of three vertices or more in one RLE, for which the parent stage has done D*D*3 crossing tests already.
// No spin, no cross-workgroup protocol.  Algorithmic bytes: every vertex is read once by measure and once per target ring that neither
// the order nor the box culls.
#include "kernels.h"
#include "nest_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

constexpr int TH = 256;
constexpr int WAVES = TH / 64;
constexpr unsigned long long NONE = ~0ull;

// ---- check ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_nest_check_rles(NestRings in, unsigned long long* __restrict__ summary)
{
    const long long k = (long long)blockIdx.x * TH + threadIdx.x;
    const long long* rr = in.rle_rings;
    if (in.n_rles == 0) {
        if (k == 0 && (rr[0] != 0 || in.n_rings != 0)) atomicMin(&summary[0], 0ull);
        return;
    }
    if (k >= in.n_rles) return;
    if ((k == 0 && rr[0] != 0) || rr[k + 1] < rr[k] || (k == in.n_rles - 1 && rr[k + 1] != in.n_rings)) atomicMin(&summary[0], (unsigned long long)k);
}

__global__ __launch_bounds__(TH) void k_nest_check_offsets(NestRings in, unsigned long long* __restrict__ summary)
{
    const long long r = (long long)blockIdx.x * TH + threadIdx.x;
    if (r >= in.n_rings) return;
    const long long a = in.ring_offsets[r], b = in.ring_offsets[r + 1];
    if (a < 0 || b < a || b - a >= (1LL << 31)) atomicMin(&summary[1], (unsigned long long)r);
}

// ---- measure ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(TH) void k_nest_measure(NestRings in, NestWork w, unsigned long long* __restrict__ summary)
{
    if (summary[0] != NONE || summary[1] != NONE) return;        // (written by the launches before this one: the offsets bound what is read here)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = (long long)blockIdx.x * WAVES + wave; r < in.n_rings; r += (long long)gridDim.x * WAVES) {      // (a wave alike)
        const long long v0 = in.ring_offsets[r];
        const int m = (int)(in.ring_offsets[r + 1] - v0);
        const int32_t* v = in.xy + 2 * v0;
        long long twice = 0;
        int x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
        bool bad = false;
        for (int i = lane; i < m; i += 64) {
            const int j = i + 1 < m ? i + 1 : 0;
            const int ax = v[2 * (long long)i], ay = v[2 * (long long)i + 1], bx = v[2 * (long long)j], by = v[2 * (long long)j + 1];
            bad |= ax < 0 || ax > NEST_COORD_MAX || ay < 0 || ay > NEST_COORD_MAX;
            twice += nest_area_term(ax, ay, bx, by);
            x0 = min(x0, ax); y0 = min(y0, ay); x1 = max(x1, ax); y1 = max(y1, ay);
        }
        twice = wave_sum(twice);
        x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
        const bool any_bad = __any(bad);
        if (lane != 0) continue;
        w.size[r] = nest_abs(twice);
        w.box[r] = make_int4(x0, y0, x1, y1);
        w.rle[r] = last_not_above((int)in.n_rles, r, [&](int i) { return in.rle_rings[i]; });      // the last of equal entries owns the ring
        if (any_bad) atomicMin(&summary[2], (unsigned long long)r);
    }
}

// ---- parent -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_nest_parent(NestRings in, NestWork w, long long* __restrict__ parent)
{
    __shared__ unsigned long long best_size[WAVES];
    __shared__ long long best_ring[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = blockIdx.x; r < in.n_rings; r += gridDim.x) {                                 // (the whole block alike)
        const long long v0 = in.ring_offsets[r];
        long long best = -1;
        unsigned long long best_a = 0;
        if (in.ring_offsets[r + 1] > v0) {                       // the ring has a first vertex: a probe
            const int X0 = in.xy[2 * v0], Y0 = in.xy[2 * v0 + 1];
            const unsigned long long ar = w.size[r];
            const int k = w.rle[r];
            const long long q1 = in.rle_rings[k + 1];
            for (long long q = in.rle_rings[k] + wave; q < q1; q += WAVES) {                         // (a wave alike)
                if (q == r) continue;
                const unsigned long long aq = w.size[q];
                if (!nest_outranks(aq, q, ar, r) || (best >= 0 && !nest_closer(aq, q, best_a, best))) continue;
                const int4 b = w.box[q];
                if (!(b.x <= X0 && X0 < b.z && b.y <= Y0 && Y0 < b.w)) continue;
                const long long u0 = in.ring_offsets[q];
                const int m = (int)(in.ring_offsets[q + 1] - u0);
                if (m < 3) continue;
                const int32_t* v = in.xy + 2 * u0;
                bool odd = false;
                for (int i = lane; i < m; i += 64) {
                    const int j = i + 1 < m ? i + 1 : 0;
                    odd ^= nest_crosses(v[2 * (long long)i], v[2 * (long long)i + 1], v[2 * (long long)j], v[2 * (long long)j + 1], X0, Y0);
                }
                if (__popcll(__ballot(odd)) & 1) { best = q; best_a = aq; }
            }
        }
        if (lane == 0) { best_size[wave] = best_a; best_ring[wave] = best; }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long p = -1;
            unsigned long long pa = 0;
            for (int i = 0; i < WAVES; ++i)
                if (best_ring[i] >= 0 && (p < 0 || nest_closer(best_size[i], best_ring[i], pa, p))) { p = best_ring[i]; pa = best_size[i]; }
            parent[r] = p;
        }
        __syncthreads();                                         // the next ring reuses the LDS
    }
}

// ---- depth ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_nest_depth(long long n_rings, const long long* __restrict__ parent, int32_t* __restrict__ depth, NestWork w)
{
    const long long r = (long long)blockIdx.x * TH + threadIdx.x;
    if (r >= n_rings) return;
    int d = 0;
    for (long long p = parent[r]; p >= 0 && d < n_rings; p = parent[p]) ++d;                         // (a forest: d < n_rings always)
    depth[r] = d;
    w.shell[r] = (d & 1) ? 0u : 1u;
    if (d & 1) atomicAdd(&w.holes[parent[r]], 1u);
}

__global__ __launch_bounds__(TH) void k_nest_sizes(long long n_rings, NestWork w)
{
    const long long r = (long long)blockIdx.x * TH + threadIdx.x;
    if (r < n_rings) w.rings[r] = w.shell[r] ? 1u + w.holes[r] : 0u;
}

// exclusive prefix of in[0 .. n) -> out[0 .. n]; one block
__global__ __launch_bounds__(1024) void k_nest_scan(const uint32_t* __restrict__ in, long long n, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(in, n, out, buf);
}

// ---- place ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_nest_place(NestRings in, NestWork w, const long long* __restrict__ parent, long long* __restrict__ poly_rings,
                                                   long long* __restrict__ ring_order)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = in.n_rings;
    if (blockIdx.x == 0 && threadIdx.x == 0) poly_rings[w.polygon[n]] = (long long)w.start[n];      // the end of the last polygon: n_rings
    for (long long r = (long long)blockIdx.x * WAVES + wave; r < n; r += (long long)gridDim.x * WAVES) {              // (a wave alike)
        if (w.shell[r]) {
            if (lane == 0) {
                poly_rings[w.polygon[r]] = (long long)w.start[r];
                ring_order[w.start[r]] = r;
            }
            continue;
        }
        const long long s = parent[r];
        int before = 0;                                          // the siblings with a smaller index
        for (long long base = in.rle_rings[w.rle[r]]; base < r; base += 64) {
            const long long q = base + lane;
            before += __popcll(__ballot(q < r && parent[q] == s));
        }
        const long long at = (long long)w.start[s] + 1 + before;
        if (lane == 0 && at < n) ring_order[at] = r;             // (always: the shell's size counted this ring)
    }
}

__global__ __launch_bounds__(TH) void k_nest_rles(NestRings in, NestWork w, long long* __restrict__ rle_polys)
{
    const long long k = (long long)blockIdx.x * TH + threadIdx.x;
    if (k <= in.n_rles) rle_polys[k] = (long long)w.polygon[in.rle_rings[k]];
}

dim3 flat(long long n) { return dim3((unsigned)((n + TH - 1) / TH)); }
// one workgroup per ring (per_ring) or one wave per ring (per_wave) up to a grid that fills the device many times over; the rest by striding
dim3 per_ring(long long n) { return dim3((unsigned)(n < (1LL << 20) ? n : (1LL << 20))); }
dim3 per_wave(long long n) { return per_ring((n + WAVES - 1) / WAVES); }

}  // namespace

void nest_measure_forward(hipStream_t s, const NestRings& in, const NestWork& w, unsigned long long* summary)
{
    HIP_CHECK(hipMemsetAsync(summary, 0xff, 3 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_nest_check_rles, flat(in.n_rles > 0 ? in.n_rles : 1), dim3(TH), 0, s, in, summary);
    if (in.n_rings > 0) {
        hipLaunchKernelGGL(k_nest_check_offsets, flat(in.n_rings), dim3(TH), 0, s, in, summary);
        hipLaunchKernelGGL(k_nest_measure, per_wave(in.n_rings), dim3(TH), 0, s, in, w, summary);
    }
    HIP_CHECK(hipGetLastError());
}

void nest_forward(hipStream_t s, const NestRings& in, const NestWork& w, long long* parent, int32_t* depth, long long* rle_polys, long long* poly_rings,
                  long long* ring_order)
{
    const long long n = in.n_rings;
    if (n <= 0) return;
    HIP_CHECK(hipMemsetAsync(w.holes, 0, (size_t)n * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_nest_parent, per_ring(n), dim3(TH), 0, s, in, w, parent);
    hipLaunchKernelGGL(k_nest_depth, flat(n), dim3(TH), 0, s, n, parent, depth, w);
    hipLaunchKernelGGL(k_nest_scan, dim3(1), dim3(1024), 0, s, w.shell, n, w.polygon);
    hipLaunchKernelGGL(k_nest_sizes, flat(n), dim3(TH), 0, s, n, w);
    hipLaunchKernelGGL(k_nest_scan, dim3(1), dim3(1024), 0, s, w.rings, n, w.start);
    hipLaunchKernelGGL(k_nest_place, per_wave(n), dim3(TH), 0, s, in, w, parent, poly_rings, ring_order);
    hipLaunchKernelGGL(k_nest_rles, flat(in.n_rles + 1), dim3(TH), 0, s, in, w, rle_polys);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
