// kernels_jpeg_entropy.hip — the entropy stage of the JPEG decoder on the device: self-synchronising parallel Huffman decoding
// (Weissenberger & Schmidt, ICPP 2018) over a ragged batch.  The decoding step and one unit's turn around it (byte range, context, sink,
// the writing pass's verdict) are jpeg_entropy.h's, shared with the host model (jpeg_entropy_host.cpp), which runs these phases launch
// for launch:
//   k_ent_sync  x launches   one thread per unit, one workgroup per 256 units of ONE file, the file's Huffman tables in LDS.  A round
//                            decodes every unit from the state its predecessor left in the round before (LDS, one barrier a round)
//                            until nothing in the workgroup changes; a workgroup's first unit takes the state the workgroup before it
//                            left in the PREVIOUS launch.  A workgroup whose entry state did not change has nothing to do.
//   k_ent_scan               exclusive scan of the blocks completed per unit (one block)
//   k_ent_write              every unit once more from its now-known state, writing coefficients (the DC as its difference) into the
//                            layout k_jpeg_idct reads, and checking that it reproduces the recorded state and count
//   k_ent_dc                 the DC predictors: one wave per (segment, component), inclusive scan modulo 2^16
// Phases exchange data across launch boundaries, or inside a workgroup through LDS and barriers; nothing waits for another workgroup.
// Every loop is bounded by the unit size, the round cap or a count from the plan; every read of the stream is below its segment's end.
#include "kernels_jpeg_entropy.h"

namespace mrcnn {

using namespace jpeg;

namespace {

constexpr int TAB_WORDS = 6 * (int)sizeof(HuffTable) / 4;

__device__ inline void stage_tables(const EntFile& f, uint32_t* s_tab)
{
    const uint32_t* src = reinterpret_cast<const uint32_t*>(f.tab);
    for (int i = threadIdx.x; i < TAB_WORDS; i += ENT_WG_UNITS) s_tab[i] = src[i];
}

}  // namespace

__global__ __launch_bounds__(ENT_WG_UNITS) void k_ent_sync(JpegEntBuffers b, int launch)
{
    __shared__ uint32_t s_tab[TAB_WORDS];
    __shared__ ent_state s_st[2][ENT_WG_UNITS];
    const int w = blockIdx.x, t = threadIdx.x;
    const EntWg g = b.wgs[w];
    const EntFile& f = b.files[g.file];
    const int cur = launch & 1, prev = cur ^ 1;
    const ent_state entry = launch > 0 && w > f.wg0 ? b.wg_exit[(size_t)prev * b.nwg + w - 1] : ENT_INVALID;
    if (launch > 0 && b.wg_flags[2 * w] && entry == b.wg_entry[w]) {           // (uniform over the workgroup: nothing here has changed)
        if (t == 0) b.wg_exit[(size_t)cur * b.nwg + w] = b.wg_exit[(size_t)prev * b.nwg + w];
        return;
    }
    stage_tables(f, s_tab);
    const bool live = t < g.count;
    const int u = g.unit0 + t;
    EntUnit q = {};
    EntCtx c = {};
    ent_state guess = ENT_INVALID;
    int cnt = 0;
    if (live) {
        const EntSeg s = b.segs[b.unit_seg[u]];
        q = ent_unit(s, u, b.unit_bytes);
        c = ent_ctx(f, s, b.bytes + f.byte0, reinterpret_cast<const HuffTable*>(s_tab), kZigzag);
        guess = ent_guess(c.data, c.b0, q.ub);
        cnt = (int)b.count[u];
    }
    s_st[0][t] = live ? b.state[u] : ENT_INVALID;
    __syncthreads();
    int at = 0, any = 1, n = 0;
    ent_state last_in = ENT_INVALID;
    while (n < b.inner_rounds && any) {
        int changed = 0;
        if (live) {
            ent_state in = q.first ? ent_pack(c.b0 * 8, 0, 0) : (t == 0 ? entry : s_st[at][t - 1]);
            if (in == ENT_INVALID) in = guess;
            if (n > 0 && in == last_in) {                  // the same question as in the round before: the same answer
                s_st[at ^ 1][t] = s_st[at][t];
            } else {
                const EntResult r = decode_unit(c, q.ub, q.ue, in, nullptr);
                changed = r.state != s_st[at][t] || r.blocks != cnt;
                s_st[at ^ 1][t] = r.state;
                cnt = r.blocks;
                last_in = in;
            }
        }
        any = __syncthreads_or(changed);
        at ^= 1;
        ++n;
    }
    if (live) { b.state[u] = s_st[at][t]; b.count[u] = (uint32_t)cnt; }
    if (t == g.count - 1) {
        const ent_state out = s_st[at][t];
        b.wg_exit[(size_t)cur * b.nwg + w] = out;
        if (any || launch == 0 || out != b.wg_exit[(size_t)prev * b.nwg + w]) atomicMax(&b.verdict[2 * g.file + 1], launch + 1);
    }
    if (t == 0) {
        b.wg_entry[w] = entry;
        b.wg_flags[2 * w] = !any;
        const int total = b.wg_flags[2 * w + 1] + n;
        b.wg_flags[2 * w + 1] = total;
        atomicMax(&b.verdict[2 * b.batch], total);
        if (launch == b.launches - 1 && any && f.nunits > 1) atomicOr(&b.verdict[2 * g.file], (int)ENT_BAD_SYNC);
    }
}

// exclusive scan of count[0 .. n) -> prefix[0 .. n], prefix[n] = the sum; one block of 1024
__global__ __launch_bounds__(1024) void k_ent_scan(const uint32_t* __restrict__ count, int n, uint32_t* __restrict__ prefix)
{
    __shared__ uint32_t buf[2][1024];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < n; base += 4096) {
        const int i0 = base + 4 * t;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? count[i0 + k] : 0;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        int cur = 0;
        buf[0][t] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            buf[cur ^ 1][t] = buf[cur][t] + (t >= d ? buf[cur][t - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        uint32_t run = carry + buf[cur][t] - mine;
        const uint32_t total = buf[cur][1023];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) prefix[i0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (t == 0) prefix[n] = carry;
}

__global__ __launch_bounds__(ENT_WG_UNITS) void k_ent_write(JpegEntBuffers b, int16_t* __restrict__ coef)
{
    __shared__ uint32_t s_tab[TAB_WORDS];
    __shared__ uint8_t s_zz[64];
    const int w = blockIdx.x, t = threadIdx.x;
    const EntWg g = b.wgs[w];
    const EntFile& f = b.files[g.file];
    stage_tables(f, s_tab);
    if (t < 64) s_zz[t] = kZigzag[t];
    __syncthreads();
    if (t >= g.count) return;
    const int u = g.unit0 + t;
    const EntSeg s = b.segs[b.unit_seg[u]];
    const EntCtx c = ent_ctx(f, s, b.bytes + f.byte0, reinterpret_cast<const HuffTable*>(s_tab), s_zz);
    const uint32_t p0 = b.prefix[s.unit0];
    const int bad = ent_write_unit(c, f, s, u, b.unit_bytes, b.state, b.prefix[u] - p0, b.prefix[u + 1] - p0, coef);
    if (bad) atomicOr(&b.verdict[2 * g.file], bad);
}

__global__ __launch_bounds__(256) void k_ent_dc(JpegEntBuffers b, int16_t* __restrict__ coef)
{
    const int wave = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (wave >= b.nsegs * 3) return;
    const int si = wave / 3, comp = wave - si * 3;
    const EntSeg s = b.segs[si];
    const EntFile& f = b.files[s.file];
    if (comp >= f.ncomp) return;
    const EntSink k = ent_sink(f, coef);
    const int per = comp == 0 ? f.nluma : 1;
    const long long first_mcu = s.first_block / f.bpm, mcu_blocks = (long long)f.mcus_x * f.mcus_y * f.bpm;
    const int total = s.nblocks / f.bpm * per;
    unsigned carry = 0;
    for (int base = 0; base < total; base += 64) {
        const int j = base + lane;
        unsigned v = 0;
        long long at = -1;
        if (j < total) {
            const long long seq = (first_mcu + j / per) * f.bpm + (comp == 0 ? j % per : f.nluma + comp - 1);
            if (seq < mcu_blocks) {
                at = ent_block_index(k, seq, f.bpm, f.nluma) * 64;
                v = (uint16_t)coef[at];
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned x = __shfl_up(v, d);
            if (lane >= d) v += x;
        }
        v += carry;
        if (at >= 0) coef[at] = (int16_t)(uint16_t)v;
        carry = __shfl(v, 63) & 0xFFFFu;
    }
}

void jpeg_entropy_forward(hipStream_t s, const JpegEntBuffers& b, int16_t* coef, long long total_blocks)
{
    HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)total_blocks * 64 * sizeof(int16_t), s));
    if (b.nwg == 0) return;
    for (int launch = 0; launch < b.launches; ++launch) {
        hipLaunchKernelGGL(k_ent_sync, dim3(b.nwg), dim3(ENT_WG_UNITS), 0, s, b, launch);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ent_scan, dim3(1), dim3(1024), 0, s, b.count, b.nunits, b.prefix);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ent_write, dim3(b.nwg), dim3(ENT_WG_UNITS), 0, s, b, coef);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ent_dc, dim3((b.nsegs * 3 + 3) / 4), dim3(256), 0, s, b, coef);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
