// kernels_simplify.hip — polygon rings simplified by Douglas-Peucker (mrcnn_polygons_simplify).  simplify_host.cpp, which recurses with
// a stack, is the definition these kernels must equal, and simplify_rule.h is what the two share.  The subproblems of the recursion are
// independent, so all chains of a ring are handled at once, level by level, and the kept set is the same.
//
//   check   the offsets per ring and every coordinate; the caller reads one summary back before anything is written
//   count   one workgroup per ring.  Every vertex that is neither kept nor dropped yet knows the chain (a, b) it lies in.  A round: every
//           such vertex offers simp_key(distance, position) to its chain's slot (a 64-bit maximum: the largest distance, the smallest
//           position); barrier; it reads the winner and runs the threshold test, then it is dropped with its whole chain, or is the
//           winner and kept, or takes the winner as its new a or b.  The slots have two sides: a round clears, on the other side, the
//           slots the next round offers to.  A ring of at most SIMPLIFY_LDS_VERTICES vertices lives in LDS (coordinates, chains and slots:
//           28 KiB), a larger one in its own carve of a global scratch, the threads striding over it.
//   scan    the rings' counts -> out_ring_offsets; the caller reads the total back for the capacity check
//   write   one workgroup per ring compacts the kept vertices to their places and sums the shoelace terms of the simplified ring
//
// The test is run by every vertex of a chain, not once per chain: it is a dozen integer multiplications, and one more barrier per round
// to hand a verdict round would cost more.  No spin, no cross-workgroup protocol: a workgroup only ever waits at its own barriers.
// Algorithmic bytes per input vertex: 8 read + 1 written (keep), 1 + 8 read again; per output vertex 8 + 8 written, 8 read for the area.
#include "kernels.h"
#include "scan_device.h"
#include "simplify_rule.h"

namespace mrcnn {
namespace {

constexpr int TH = 256;
constexpr int LDS_N = SIMPLIFY_LDS_VERTICES;
constexpr unsigned long long NONE = ~0ull;
static_assert(LDS_N >= 4 && LDS_N < 65536, "MRCNN_SIMPLIFY_LDS_VERTICES: a chain's two ends are kept in 16 bits each");

// ---- check ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_simplify_check_offsets(SimplifyRings in, unsigned long long* __restrict__ summary)
{
    const long long r = (long long)blockIdx.x * TH + threadIdx.x;
    if (r >= in.n_rings) return;
    const long long a = in.ring_offsets[r], b = in.ring_offsets[r + 1];
    if (a < 0 || b < a || b - a >= (1LL << 31)) atomicMin(&summary[0], (unsigned long long)r);
    else atomicMax(&summary[2], (unsigned long long)(b - a));
    if (r == in.n_rings - 1) summary[3] = (unsigned long long)b;
}

// a fixed grid strides over the coordinates; only a bad one looks for its ring
__global__ __launch_bounds__(TH) void k_simplify_check_xy(SimplifyRings in, unsigned long long* __restrict__ summary)
{
    if (summary[0] != NONE || in.n_rings <= 0) return;           // (written by the launch before this one: the offsets bound what is read here)
    const long long* off = in.ring_offsets;
    const long long first = 2 * off[0], last = 2 * off[in.n_rings];
    for (long long v = first + (long long)blockIdx.x * TH + threadIdx.x; v < last; v += (long long)gridDim.x * TH) {
        const int32_t c = in.xy[v];
        if (c >= 0 && c <= SIMP_COORD_MAX) continue;
        // the last of equal offsets at or below the vertex is the ring that owns it (n_rings < 2^31)
        const int r = last_not_above((int)in.n_rings, v >> 1, [&](int i) { return off[i]; });
        atomicMin(&summary[1], (unsigned long long)r);
    }
}

// ---- a ring's storage ----------------------------------------------------------------------------------------------------------
// Both kinds answer: x(i), y(i) for 0 <= i <= m (vertex m is vertex 0 again); chain(i, &a, &b) / set_chain / retire for the vertex's own
// state, which only the thread that owns the vertex touches; offer / winner / clear for the slot of the chain that starts at a, side 0 or 1.
struct RingLds {
    int32_t x[LDS_N + 1], y[LDS_N + 1];
    uint32_t chain[LDS_N];                                       // (a << 16) | b, b <= LDS_N; all ones: neither in a chain any more
    unsigned long long slot[2][LDS_N];
};

struct InLds {
    RingLds* s;
    __device__ int x(int i) const { return s->x[i]; }
    __device__ int y(int i) const { return s->y[i]; }
    __device__ bool chain(int i, int* a, int* b) const
    {
        const uint32_t w = s->chain[i];
        *a = (int)(w >> 16); *b = (int)(w & 0xffffu);
        return w != ~0u;
    }
    __device__ void set_chain(int i, int a, int b) { s->chain[i] = ((uint32_t)a << 16) | (uint32_t)b; }
    __device__ void retire(int i) { s->chain[i] = ~0u; }
    __device__ void offer(int side, int a, unsigned long long key) { atomicMax(&s->slot[side][a], key); }
    __device__ unsigned long long winner(int side, int a) const { return s->slot[side][a]; }
    __device__ void clear(int side, int a) { s->slot[side][a] = 0; }
};

// The ring's carve of the global scratch: entries v0 .. v0 + m of chain and of the two sides.  The slots are written and read with
// device-scope atomics, between the workgroup's barriers: a workgroup's own writes, seen by its other waves.
struct InGlobal {
    const int32_t* xy;                                           // the ring's first vertex
    int m;
    unsigned long long *chain_, *slot[2];
    __device__ int x(int i) const { return xy[2 * (long long)(i == m ? 0 : i)]; }
    __device__ int y(int i) const { return xy[2 * (long long)(i == m ? 0 : i) + 1]; }
    __device__ bool chain(int i, int* a, int* b) const
    {
        const unsigned long long w = chain_[i];
        *a = (int)(w >> 32); *b = (int)(uint32_t)w;
        return w != NONE;
    }
    __device__ void set_chain(int i, int a, int b) { chain_[i] = ((unsigned long long)(uint32_t)a << 32) | (uint32_t)b; }
    __device__ void retire(int i) { chain_[i] = NONE; }
    __device__ void offer(int side, int a, unsigned long long key) { atomicMax(&slot[side][a], key); }
    __device__ unsigned long long winner(int side, int a) const { return __hip_atomic_load(&slot[side][a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void clear(int side, int a) { __hip_atomic_store(&slot[side][a], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// The rule on one ring of m >= 3 vertices; every thread of the block calls it.  keep: the ring's m flags.  Returns how many vertices
// this thread kept.
template <class Ring>
__device__ int simplify_ring(Ring R, int m, unsigned long long E, uint8_t* __restrict__ keep)
{
    const int t = threadIdx.x;
    for (int i = t; i < m; i += TH) { R.clear(0, i); R.clear(1, i); }
    __syncthreads();
    // the second anchor: the same maximum, over the squared distances from vertex 0
    const int x0 = R.x(0), y0 = R.y(0);
    for (int i = t; i < m; i += TH) R.offer(0, 0, simp_key(simp_dist2(x0, y0, R.x(i), R.y(i)), i));
    __syncthreads();
    const int f = simp_key_position(R.winner(0, 0));
    __syncthreads();                                             // every thread has read it
    if (t == 0) R.clear(0, 0);
    int kept = 0;
    for (int i = t; i < m; i += TH) {
        const bool anchor = i == 0 || i == f;
        keep[i] = anchor ? 1 : 0;
        kept += anchor ? 1 : 0;
        if (anchor) R.retire(i);
        else if (i < f) R.set_chain(i, 0, f);
        else R.set_chain(i, f, m);
    }
    __syncthreads();
    // Every round either drops a whole chain or keeps one more vertex of it, so no chain is left after at most m rounds: the loop ends.
    for (int side = 0;; side ^= 1) {
        bool live = false;
        for (int i = t; i < m; i += TH) {
            int a, b;
            if (!R.chain(i, &a, &b)) continue;
            live = true;
            R.offer(side, a, simp_key(simp_distance(R.x(a), R.y(a), R.x(b), R.y(b), R.x(i), R.y(i)), i));
        }
        if (!__syncthreads_or(live ? 1 : 0)) break;              // (the whole block alike)
        for (int i = t; i < m; i += TH) {
            int a, b;
            if (!R.chain(i, &a, &b)) continue;
            const unsigned long long win = R.winner(side, a);
            const int k = simp_key_position(win);
            if (!simp_keeps(simp_key_distance(win), E, R.x(a), R.y(a), R.x(b), R.y(b))) R.retire(i);
            else if (i == k) { keep[i] = 1; ++kept; R.retire(i); }
            else if (i < k) { R.set_chain(i, a, k); R.clear(side ^ 1, a); }
            else { R.set_chain(i, k, b); R.clear(side ^ 1, k); }
        }
        __syncthreads();
    }
    return kept;
}

__global__ __launch_bounds__(TH) void k_simplify_count(SimplifyRings in, unsigned long long E, SimplifyWork w)
{
    __shared__ RingLds lds;
    __shared__ int total;
    const int t = threadIdx.x;
    for (long long r = blockIdx.x; r < in.n_rings; r += gridDim.x) {
        const long long v0 = in.ring_offsets[r];
        const long long mm = in.ring_offsets[r + 1] - v0;
        if (v0 < 0 || mm <= 0 || mm >= (1LL << 31)) {            // (an empty ring; the others cannot be: the offsets were checked.  The whole block alike)
            if (t == 0) w.count[r] = 0;
            continue;
        }
        const int m = (int)mm;
        uint8_t* keep = w.keep + v0;
        if (m <= 2) {
            if (t < m) keep[t] = 1;
            if (t == 0) w.count[r] = (uint32_t)m;
            continue;
        }
        if (t == 0) total = 0;
        int kept;
        if (m <= LDS_N) {
            for (int i = t; i < m; i += TH) { lds.x[i] = in.xy[2 * (v0 + i)]; lds.y[i] = in.xy[2 * (v0 + i) + 1]; }
            if (t == 0) { lds.x[m] = in.xy[2 * v0]; lds.y[m] = in.xy[2 * v0 + 1]; }
            __syncthreads();
            kept = simplify_ring(InLds{&lds}, m, E, keep);
        } else {
            if (!w.chain) continue;                              // (cannot be: the caller sized the scratch by the largest ring)
            __syncthreads();                                     // total is cleared
            kept = simplify_ring(InGlobal{in.xy + 2 * v0, m, w.chain + v0, {w.slot_a + v0, w.slot_b + v0}}, m, E, keep);
        }
        atomicAdd(&total, kept);
        __syncthreads();
        if (t == 0) w.count[r] = (uint32_t)total;
        __syncthreads();                                         // the next ring reuses total and the LDS
    }
}

// exclusive prefix of count[0 .. n) -> out[0 .. n]; one block
__global__ __launch_bounds__(1024) void k_simplify_scan(const uint32_t* __restrict__ in, long long n, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(in, n, out, buf);
}

// ---- write ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TH) void k_simplify_write(SimplifyRings in, SimplifyWork w, const long long* __restrict__ out_off, long long n_out,
                                                       long long* __restrict__ out_areas2, int32_t* out_xy, long long* __restrict__ out_src)
{
    __shared__ int wave_n[4];
    __shared__ unsigned long long area;
    const int t = threadIdx.x;
    for (long long r = blockIdx.x; r < in.n_rings; r += gridDim.x) {
        const long long v0 = in.ring_offsets[r], m = in.ring_offsets[r + 1] - v0;
        const long long o0 = out_off[r], cnt = out_off[r + 1] - o0;
        if (t == 0) area = 0;
        __syncthreads();
        long long run = 0;
        for (long long base = 0; base < m; base += TH) {         // (the whole block alike)
            const long long i = base + t;
            const bool kp = i < m && w.keep[v0 + i] != 0;
            int n = 0;
            const long long at = run + compact_256(kp, wave_n, &n);
            if (kp && at < cnt && o0 + at < n_out) {             // (always, for the flags the count launch wrote)
                out_xy[2 * (o0 + at)] = in.xy[2 * (v0 + i)];
                out_xy[2 * (o0 + at) + 1] = in.xy[2 * (v0 + i) + 1];
                if (out_src) out_src[o0 + at] = v0 + i;
            }
            run += n;
            __syncthreads();
        }
        if (!out_areas2) continue;
        // twice the signed area: the shoelace terms of the ring as this workgroup has just written it
        const auto at = [&](long long j) { return (long long)__hip_atomic_load(&out_xy[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        long long sum = 0;
        if (o0 + cnt <= n_out)
            for (long long j = t; j < cnt; j += TH) {
                const long long p = 2 * (o0 + j), q = 2 * (o0 + (j + 1 < cnt ? j + 1 : 0));
                sum += at(p) * at(q + 1) - at(q) * at(p + 1);
            }
        atomicAdd(&area, (unsigned long long)sum);
        __syncthreads();
        if (t == 0) out_areas2[r] = (long long)area;
        __syncthreads();
    }
}

dim3 flat(long long n) { return dim3((unsigned)((n + TH - 1) / TH)); }
// one workgroup per ring up to a grid that fills the device many times over; the rest by striding
dim3 per_ring(long long n) { return dim3((unsigned)(n < (1LL << 20) ? n : (1LL << 20))); }

}  // namespace

void simplify_check_forward(hipStream_t s, const SimplifyRings& in, unsigned long long* summary)
{
    HIP_CHECK(hipMemsetAsync(summary, 0xff, 2 * sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(summary + 2, 0, 2 * sizeof(unsigned long long), s));
    if (in.n_rings <= 0) return;
    hipLaunchKernelGGL(k_simplify_check_offsets, flat(in.n_rings), dim3(TH), 0, s, in, summary);
    hipLaunchKernelGGL(k_simplify_check_xy, dim3(2048), dim3(TH), 0, s, in, summary);
    HIP_CHECK(hipGetLastError());
}

void simplify_count_forward(hipStream_t s, const SimplifyRings& in, unsigned long long E, const SimplifyWork& w, long long* out_ring_offsets)
{
    if (in.n_rings <= 0) return;
    hipLaunchKernelGGL(k_simplify_count, per_ring(in.n_rings), dim3(TH), 0, s, in, E, w);
    hipLaunchKernelGGL(k_simplify_scan, dim3(1), dim3(1024), 0, s, w.count, in.n_rings, reinterpret_cast<unsigned long long*>(out_ring_offsets));
    HIP_CHECK(hipGetLastError());
}

void simplify_write_forward(hipStream_t s, const SimplifyRings& in, const SimplifyWork& w, const long long* out_ring_offsets, long long n_out,
                            long long* out_areas2, int32_t* out_xy, long long* out_src_index)
{
    if (in.n_rings <= 0) return;
    hipLaunchKernelGGL(k_simplify_write, per_ring(in.n_rings), dim3(TH), 0, s, in, w, out_ring_offsets, n_out, out_areas2, out_xy, out_src_index);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
