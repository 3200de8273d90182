// kernels_conv_chain.hip — split modes: a bottleneck's `branch2c` (P: C -> 4C, + residual or fused shortcut, ReLU) and the NEXT
// block's `branch2a` (Q: 4C -> C, ReLU) as one launch (conv_dispatch.hip: conv_forward_chain).  The tile of y = P's output that a
// wave has just activated is exactly Q's activation operand for the same pixels: Q is computed from it while it is on chip, so
// the 4C-wide tensor is stored (the next block's residual) but not read back by a launch of its own.
//
// BIT-IDENTICAL to conv_forward(P); conv_forward(Q), output for output.  A wave owns 32 pixel rows and walks ALL of P's 4C columns
// in ascending chunks of 64.  The arithmetic is written ONCE, in the building blocks ahead of the kernels:
//   * chain_split_row / chain_mfma_parts — P's sums per chunk are the 128-row kernel's: K steps of 32 channels, groups of 16
//     ascending, hi / mid / lo part per group, filter fragment first;
//   * ChainTile — the wave-private 32 x 32 LDS tile of conv_epilogue_wave: accumulators in (put), rows out and back (row_get /
//     row_put), Q's activation fragments out (frag);
//   * chain_scale_shift, chain_add, chain_relu, chain_beyond_fp16 — conv_epilogue_wave's expressions on four adjacent columns (scale /
//     shift, + residual — loaded by chain_residual / chain_residual_piece, or formed from the shortcut's sums —, ReLU, the fp16-range watch);
//   * chain_piece_p (the ring form's) — one 32 x 32 piece of P through them, stored, and left in the tile as y: the stored fp32 values, which Q's step
//     splits by split_hi_mid_lo / split_hi_lo and multiplies into Q's accumulators: one running sum per output, channel groups
//     ascending — Q's own order.  k_conv_chain spells the piece (and the shortcut's, which only it has) out of the same primitives in
//     its body: called as a function it costs k_conv_chain<64, 3, SC>, which sits at its 256 registers, 12 B of scratch;
//   * chain_epilogue_q — Q's epilogue: the same piece without a residual.
// What a kernel body adds is where its FILTERS come from.  In k_conv_chain the waves of a block share no pixel and nothing
// synchronises them inside the loop; in the ring form two waves share 32 rows and split the work by role, and one block barrier per piece hands
// filter stages and P's sums over.
//   * k_conv_chain<64>: every filter of the launch resident in LDS, one persistent block of eight waves per CU — what
//     conv_forward_chain runs for C2;
//   * k_conv_chain<128>: P's activation tile (32 rows x C fp32 per wave) in LDS in the 128-row kernel's swizzled layout, both layers'
//     filter fragments straight from L2 (16 B per lane) — measured slower than the two launches, kept as the tests' bit-identity anchor;
//   * k_conv_chain_ring<256>: both layers' filters streamed through block-shared LDS stages, eight waves in two roles — what runs for C4.
#include "conv_device.h"

namespace mrcnn {

struct ChainArgs { ConvArgs p, q; const void *p_stream, *q_stream; };        // the stream images: the ring form (C = 256) only

// ---- four adjacent columns of one row: conv_epilogue_wave's expressions -------------------------------------------------------------
__device__ __forceinline__ float4 chain_scale_shift(float4 x, const float4 sc, const float4 sh)
{
    x.x = x.x * sc.x + sh.x; x.y = x.y * sc.y + sh.y; x.z = x.z * sc.z + sh.z; x.w = x.w * sc.w + sh.w;
    return x;
}
__device__ __forceinline__ float4 chain_add(float4 x, const float4 r) { x.x += r.x; x.y += r.y; x.z += r.z; x.w += r.w; return x; }
__device__ __forceinline__ float4 chain_relu(float4 x) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f); return x; }
__device__ __forceinline__ bool chain_beyond_fp16(const float4 x) { return !(fabsf(x.x) < 65504.0f) || !(fabsf(x.y) < 65504.0f) || !(fabsf(x.z) < 65504.0f) || !(fabsf(x.w) < 65504.0f); }
__device__ __forceinline__ float4 chain_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the row-wise read-back of a wave's 32 rows: eight lanes per row (columns c4 .. c4 + 3), four passes of eight rows
struct ChainRows { bool ok[4]; long mrow[4]; int c4; };
__device__ __forceinline__ ChainRows chain_rows(int row0, int M, int lane)
{
    ChainRows rw;
    rw.c4 = (lane & 7) * 4;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) { const int m = row0 + 8 * ps + (lane >> 3); rw.ok[ps] = m < M; rw.mrow[ps] = m; }
    return rw;
}

// the fp16 parts of eight fp32 activations: hi, (mid,) lo
struct ChainParts { f16x8 hi, lo, lo2; };
template <int PARTS>
__device__ __forceinline__ ChainParts chain_split(const uint4 u0, const uint4 u1)
{
    ChainParts p;
    if constexpr (PARTS == 3) split_hi_mid_lo(u0, u1, p.hi, p.lo, p.lo2);
    else { split_hi_lo(u0, u1, p.hi, p.lo); p.lo2 = p.lo; }
    return p;
}
// this lane's activation fragments of P (pixel row0 + l31, NG groups of 16 channels), split once into registers (rows beyond M: zeros)
template <int PARTS, int NG>
__device__ __forceinline__ void chain_split_row(ChainParts (&ap)[NG], const float* in, int row0, int M, int l31, int kk)
{
    const int m = row0 + l31;
    const bool m_ok = m < M;
    const float* const src = in + (long)(m_ok ? m : row0) * (NG * 16) + 8 * kk;
    uint4 u[NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        u[g][0] = u[g][1] = make_uint4(0u, 0u, 0u, 0u);
        if (m_ok) { u[g][0] = *reinterpret_cast<const uint4*>(src + g * 16); u[g][1] = *reinterpret_cast<const uint4*>(src + g * 16 + 4); }
        ap[g] = chain_split<PARTS>(u[g][0], u[g][1]);
    }
}
// one 16-channel group into N column tiles: every tile's hi part, then mid, then lo — per accumulator the 128-row kernel's order
// (NA, OFF: the N tiles are acc[OFF .. OFF + N) of a wider set)
template <int PARTS, int N, int NA = N, int OFF = 0>
__device__ __forceinline__ void chain_mfma_parts(f32x16 (&acc)[NA], const uint4 (&bv)[N], const ChainParts& pt)
{
    const f16x8 hi = pt.hi, lo = pt.lo, lo2 = pt.lo2;
    _Pragma("unroll") for (int j = 0; j < N; ++j) acc[OFF + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[j]), hi, acc[OFF + j], 0, 0, 0);
    _Pragma("unroll") for (int j = 0; j < N; ++j) acc[OFF + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[j]), lo, acc[OFF + j], 0, 0, 0);
    if constexpr (PARTS == 3)
        _Pragma("unroll") for (int j = 0; j < N; ++j) acc[OFF + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[j]), lo2, acc[OFF + j], 0, 0, 0);
}
template <int N>
__device__ __forceinline__ void chain_zero(f32x16 (&acc)[N])
{
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
}

// the wave-private 32 x 32 fp32 tile: 16-B chunk c of row r at c ^ (r & 7); one access pattern per member
// (the wave's own barriers between the patterns are the callers')
struct ChainTile {
    float* s;
    int lane;
    __device__ __forceinline__ float4* at(int r, int c) const { return reinterpret_cast<float4*>(&s[r * 32 + ((c ^ (r & 7)) << 2)]); }
    // an accumulator tile, transposing: lane l31 holds row l31's columns 8 q + 4 kk .. + 3
    __device__ __forceinline__ void put(const f32x16& acc) const
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) *at(lane & 31, 2 * q + (lane >> 5)) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    }
    // row-wise: pass ps of ChainRows
    __device__ __forceinline__ float4 row_get(int ps) const { return *at(8 * ps + (lane >> 3), lane & 7); }
    __device__ __forceinline__ void row_put(int ps, const float4 v) const { *at(8 * ps + (lane >> 3), lane & 7) = v; }
    // row l31's channels 16 g + 8 kk .. + 7 as an activation fragment, split
    template <int PARTS>
    __device__ __forceinline__ ChainParts frag(int g) const
    {
        const int c = 4 * g + 2 * (lane >> 5);
        return chain_split<PARTS>(*reinterpret_cast<const uint4*>(at(lane & 31, c)), *reinterpret_cast<const uint4*>(at(lane & 31, c + 1)));
    }
};

// the residual of a 64-column chunk (no residual: zeros); the callers request it before the chunk's K loop: every element the wave will
// overwrite, before its first store
__device__ __forceinline__ void chain_residual(float4 (&rv)[2][4], const float* res, const ChainRows& rw, int pitch, int nc)
{
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            rv[j][ps] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (res && rw.ok[ps]) rv[j][ps] = chain_ld4(res + rw.mrow[ps] * pitch + nc + j * 32 + rw.c4);
        }
}
// the ring form's view of the same rows, cheap in registers: the byte offset of (row, column c4) from the wave's first row in a tensor of `pitch`
// floats per row — a wave-uniform base pointer takes the rest.  A row beyond M is pointed at the wave's first row: its requests stay inside the
// tensor, nothing of it is stored or watched, and no other row's sums see it
struct ChainRowOffs { bool ok[4]; unsigned off[4]; };
__device__ __forceinline__ ChainRowOffs chain_row_offs(int row0, int M, int lane, int pitch)
{
    ChainRowOffs ro;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int r = 8 * ps + (lane >> 3);
        ro.ok[ps] = row0 + r < M;
        ro.off[ps] = (unsigned)((ro.ok[ps] ? r : 0) * pitch + (lane & 7) * 4) * 4u;
    }
    return ro;
}
// the residual of ONE 32-column piece (res: the piece's first column in the wave's first row), this lane's four rows, requested a whole piece
// ahead: every element the wave will overwrite, before the wave's store to it.  Four unconditional requests
__device__ __forceinline__ void chain_residual_piece(float4 (&rv)[4], const float* res, const ChainRowOffs& ro)
{
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) rv[ps] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(res) + ro.off[ps]);
}
// one 32 x 32 piece of P whose sums lie in the tile (ChainTile::put): columns n .. n + 3 of this lane's four rows, scaled and shifted (the tables in LDS), + r,
// activated, watched and stored (out: the piece's first column in the wave's first row); the tile is left holding y row-major (the stored values, same swizzle) for Q's step.  A lane rewrites exactly the
// elements it read.  FULL (no row lies beyond M) is straight-line code
template <bool FULL, bool RELU>
__device__ __forceinline__ void chain_piece_p(const ChainTile& tl, const float* scale, const float* shift, const float4 (&r)[4], const ChainRowOffs& ro, float* out, int n,
                                              bool& out_of_range)
{
    const float4 sc = chain_ld4(scale + n), sh = chain_ld4(shift + n);
    float4 xs[4];
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) xs[ps] = tl.row_get(ps);
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        float4 x = chain_add(chain_scale_shift(xs[ps], sc, sh), r[ps]);
        if (RELU) x = chain_relu(x);
        if (FULL || ro.ok[ps]) {
            out_of_range |= chain_beyond_fp16(x);
            *reinterpret_cast<float4*>(reinterpret_cast<char*>(out) + ro.off[ps]) = x;
        }
        xs[ps] = x;
    }
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) tl.row_put(ps, xs[ps]);
    __builtin_amdgcn_wave_barrier();
}
// Q's epilogue: TNQ pieces of 32 columns — scale / shift (tables in memory or in LDS), ReLU, watch, full-line stores
template <int TNQ>
__device__ __forceinline__ void chain_epilogue_q(const ChainTile& tl, const f32x16 (&acc)[TNQ], const float* scale, const float* shift, bool relu,
                                                 const ChainRows& rw, float* out, bool& out_of_range)
{
#pragma unroll
    for (int jq = 0; jq < TNQ; ++jq) {
        const int n = jq * 32 + rw.c4;
        tl.put(acc[jq]);
        __builtin_amdgcn_wave_barrier();
        const float4 sc = chain_ld4(scale + n), sh = chain_ld4(shift + n);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            float4 x = chain_scale_shift(tl.row_get(ps), sc, sh);
            if (relu) x = chain_relu(x);
            if (rw.ok[ps]) {
                out_of_range = out_of_range || chain_beyond_fp16(x);
                *reinterpret_cast<float4*>(out + rw.mrow[ps] * (TNQ * 32) + n) = x;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// C: P's input channels = Q's output columns (64: C2, 128: C3); SC: P's residual is formed from the fused shortcut convolution
// C = 64: every filter of the launch resident in LDS (W3, W1 and the shortcut's: 32 KB each, in the 128-row kernel's swizzled 64-B rows per
// K step), ONE block of eight waves per CU walking 32-row tiles of the whole tensor (a persistent grid: the filters are staged once per CU),
// and P's activation fragments split ONCE per tile into registers — no filter request leaves the CU inside the loop.
// C = 128: four waves of one tile each; P's activation tile in LDS, split per use; every filter fragment from L2.
template <int C, int PARTS, bool SC>
__global__ __launch_bounds__(C == 64 ? 512 : 256, C == 64 ? 1 : 2) void k_conv_chain(const ChainArgs ca)
{
    static_assert(C == 64 || C == 128, "C = 64: filters resident in LDS; C = 128: filters from L2");
    constexpr bool WLDS = C == 64;
    constexpr int NW = WLDS ? 8 : 4, C4 = 4 * C, KT = C / 32, TNP = 2, TNQ = C / 32;
    constexpr int A_BYTES = WLDS ? 0 : KT * 32 * 128;    // a wave's activation tile: KT sub-tiles of 32 rows x 128 B
    constexpr int W_BYTES = WLDS ? C4 * C * 2 : 0;       // one filter matrix (W3: [K step][4C rows][64 B]; W1: [K step][C rows][64 B])
    constexpr int WF_BYTES = W_BYTES * (SC ? 3 : 2);
    __shared__ __attribute__((aligned(16))) unsigned char smem[WF_BYTES + NW * (A_BYTES + 32 * 32 * 4)];
    const ConvArgs& a = ca.p;
    const ConvArgs& aq = ca.q;
    const int t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63;
    const int l31 = lane & 31, kk = lane >> 5;
    unsigned char* const As = smem + WF_BYTES + wave * A_BYTES;
    const ChainTile tl{reinterpret_cast<float*>(smem + WF_BYTES + NW * A_BYTES) + wave * (32 * 32), lane};
    const float* const in = static_cast<const float*>(a.in);
    const _Float16* const w3 = static_cast<const _Float16*>(a.wgt);
    const _Float16* const w1 = static_cast<const _Float16*>(aq.wgt);
    const float* const res = static_cast<const float*>(a.res);
    float* const out = static_cast<float*>(a.out);
    const _Float16* const wsc = static_cast<const _Float16*>(a.sc_wgt);
    const int swzb = (l31 >> 2) & 3;                     // filter rows in LDS: 16-B chunk c of row r at c ^ ((r >> 2) & 3)
    if constexpr (WLDS) {
        // rows x K fp16 -> [K step][row][64 B]
        auto stage_filter = [&](unsigned char* dst, const _Float16* src, int rows, int K) {
            const int cpr = K / 8;                       // 16-B chunks per filter row
            for (int idx = t; idx < rows * cpr; idx += NW * 64) {
                const int r = idx / cpr, ch = idx - r * cpr;
                *reinterpret_cast<uint4*>(dst + ((ch >> 2) * rows + r) * 64 + (((ch & 3) ^ ((r >> 2) & 3)) << 4)) = *reinterpret_cast<const uint4*>(src + (long)r * K + ch * 8);
            }
        };
        stage_filter(smem, w3, C4, C);
        stage_filter(smem + W_BYTES, w1, C, C4);
        if constexpr (SC) stage_filter(smem + 2 * W_BYTES, wsc, C4, C);
        __syncthreads();                                 // (the only block barrier: the waves share nothing else)
    }
    bool out_of_range = false, out_of_range_q = false;
    for (int row0 = (blockIdx.x * NW + wave) * 32; row0 < a.M; row0 += gridDim.x * NW * 32) {
    // ---- P's activation tile: -> LDS, or (C = 64) this lane's fragments straight into registers, split once (rows beyond M: zeros) ----
    ChainParts ap[WLDS ? 2 * KT : 1];
    if constexpr (WLDS) {
        chain_split_row<PARTS>(ap, in, row0, a.M, l31, kk);
    } else {
#pragma unroll
        for (int it = 0; it < C / 8; ++it) {
            const int idx = it * 64 + lane;
            const int r = idx / (C / 4), ch = idx - r * (C / 4);
            const int m = row0 + r;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m < a.M) v = *reinterpret_cast<const uint4*>(in + (long)m * C + ch * 4);
            *reinterpret_cast<uint4*>(As + (ch >> 3) * 4096 + r * 128 + (((ch & 7) ^ ((r >> 1) & 7)) << 4)) = v;
        }
        __builtin_amdgcn_wave_barrier();
    }

    const int swz = (l31 >> 1) & 7;
    const unsigned char* const la = As + l31 * 128;
    const int ca0 = ((0 + 2 * kk) ^ swz) << 4, ca1 = ((1 + 2 * kk) ^ swz) << 4, ca2 = ((4 + 2 * kk) ^ swz) << 4, ca3 = ((5 + 2 * kk) ^ swz) << 4;
    const ChainRows rw = chain_rows(row0, a.M, lane);
    const bool relu = a.act == ACT_RELU;

    // fused shortcut: this lane's pixel of the shortcut's input (a strided 1x1: no padding)
    const float* sc_row = nullptr;
    bool sc_ok = false;
    if constexpr (SC) {
        const int m = row0 + l31;
        sc_ok = m < a.M;
        const int ohw = a.OH * a.OW;
        const int mm = sc_ok ? m : 0;
        const int b = mm / ohw, rem = mm - b * ohw;
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        sc_row = static_cast<const float*>(a.sc_in) + (long)b * a.sc_in_sB + (long)(oh * a.sc_stride) * a.sc_in_sH + (long)(ow * a.sc_stride) * a.sc_in_sW + 8 * kk;
    }
    // C = 64: the lane's 64 shortcut-input channels, loaded once per tile (split again per column chunk: no registers for the parts)
    uint4 xr[SC && WLDS ? C / 4 : 1];
    if constexpr (SC && WLDS) {
#pragma unroll
        for (int i = 0; i < C / 4; ++i) {
            xr[i] = make_uint4(0u, 0u, 0u, 0u);
            if (sc_ok) xr[i] = *reinterpret_cast<const uint4*>(sc_row + (i >> 1) * 16 + (i & 1) * 4);
        }
    }

    f32x16 accQ[TNQ];
    chain_zero(accQ);
    for (int nc = 0; nc < C4; nc += TNP * 32) {
        float4 rv[TNP][4];                               // P's residual: loaded here, or (SC) formed piece by piece from the shortcut's sums
        if constexpr (!SC) chain_residual(rv, res, rw, C4, nc);
        f32x16 accP[TNP], accS[TNP];
        chain_zero(accP);
        chain_zero(accS);
        // ---- P: K steps of 32 channels, two groups of 16 each ------------------------------------------------------
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                uint4 bv[TNP];
                if constexpr (WLDS) {
#pragma unroll
                    for (int j = 0; j < TNP; ++j) bv[j] = *reinterpret_cast<const uint4*>(smem + (kt * C4 + nc + j * 32 + l31) * 64 + (((2 * g + kk) ^ swzb) << 4));
                    chain_mfma_parts<PARTS, TNP>(accP, bv, ap[2 * kt + g]);
                } else {
                    const uint4 u0 = *reinterpret_cast<const uint4*>(la + kt * 4096 + (g ? ca2 : ca0));
                    const uint4 u1 = *reinterpret_cast<const uint4*>(la + kt * 4096 + (g ? ca3 : ca1));
#pragma unroll
                    for (int j = 0; j < TNP; ++j) bv[j] = *reinterpret_cast<const uint4*>(w3 + (long)(nc + j * 32 + l31) * C + kt * 32 + g * 16 + 8 * kk);
                    chain_mfma_parts<PARTS, TNP>(accP, bv, chain_split<PARTS>(u0, u1));
                }
            }
        }
        if constexpr (SC) {
            // the shortcut's own sums, from zero: its channel groups ascending (fragments straight from memory)
            for (int g = 0; g < (WLDS ? C / 16 : a.sc_Cin / 16); ++g) {
                uint4 u0 = make_uint4(0u, 0u, 0u, 0u), u1 = u0;
                if constexpr (WLDS) { u0 = xr[2 * g]; u1 = xr[2 * g + 1]; }
                else if (sc_ok) { u0 = *reinterpret_cast<const uint4*>(sc_row + g * 16); u1 = *reinterpret_cast<const uint4*>(sc_row + g * 16 + 4); }
                uint4 bv[TNP];
#pragma unroll
                for (int j = 0; j < TNP; ++j) {
                    if constexpr (WLDS) bv[j] = *reinterpret_cast<const uint4*>(smem + 2 * W_BYTES + ((g >> 1) * C4 + nc + j * 32 + l31) * 64 + (((2 * (g & 1) + kk) ^ swzb) << 4));
                    else bv[j] = *reinterpret_cast<const uint4*>(wsc + (long)(nc + j * 32 + l31) * a.sc_Cin + g * 16 + 8 * kk);
                }
                chain_mfma_parts<PARTS, TNP>(accS, bv, chain_split<PARTS>(u0, u1));
            }
        }
        // ---- epilogue of the chunk, piece by piece; each piece is one K step of Q -------------------------------------
#pragma unroll
        for (int j = 0; j < TNP; ++j) {
            const int n = nc + j * 32 + rw.c4;
            if constexpr (SC) {
                // the shortcut's piece: its sums -> the residual values of P's piece, with their watch
                tl.put(accS[j]);
                __builtin_amdgcn_wave_barrier();
                const float4 sc2 = chain_ld4(a.sc_scale + n), sh2 = chain_ld4(a.sc_shift + n);
#pragma unroll
                for (int ps = 0; ps < 4; ++ps) {
                    rv[j][ps] = chain_scale_shift(tl.row_get(ps), sc2, sh2);
                    out_of_range = out_of_range || chain_beyond_fp16(rv[j][ps]);
                }
                __builtin_amdgcn_wave_barrier();
            }
            // P's piece: scaled, shifted, + residual, activated, watched and stored; the tile is left holding y row-major for Q's step
            tl.put(accP[j]);
            __builtin_amdgcn_wave_barrier();
            const float4 sc = chain_ld4(a.scale + n), sh = chain_ld4(a.shift + n);
            float4 xs[4];
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                float4 x = chain_scale_shift(tl.row_get(ps), sc, sh);
                if (SC || res) x = chain_add(x, rv[j][ps]);
                if (relu) x = chain_relu(x);
                if (rw.ok[ps]) {
                    out_of_range = out_of_range || chain_beyond_fp16(x);
                    *reinterpret_cast<float4*>(out + rw.mrow[ps] * C4 + n) = x;
                }
                xs[ps] = x;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) tl.row_put(ps, xs[ps]);
            __builtin_amdgcn_wave_barrier();
            // ---- Q: the K step of channels nc + 32 j .. + 31 ---------------------------------------------------------
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                uint4 bq[TNQ];
#pragma unroll
                for (int jq = 0; jq < TNQ; ++jq) {
                    if constexpr (WLDS) bq[jq] = *reinterpret_cast<const uint4*>(smem + W_BYTES + ((nc / 32 + j) * C + jq * 32 + l31) * 64 + (((2 * g + kk) ^ swzb) << 4));
                    else bq[jq] = *reinterpret_cast<const uint4*>(w1 + (long)(jq * 32 + l31) * C4 + nc + j * 32 + g * 16 + 8 * kk);
                }
                chain_mfma_parts<PARTS, TNQ>(accQ, bq, tl.template frag<PARTS>(g));
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    chain_epilogue_q(tl, accQ, aq.scale, aq.shift, aq.act == ACT_RELU, rw, static_cast<float*>(aq.out), out_of_range_q);
    }          // (the wave's next 32-row tile)
    if (a.range_flag && out_of_range) atomicOr(a.range_flag, 1);
    if (aq.range_flag && out_of_range_q) atomicOr(aq.range_flag, 1);
}

// The ring form (C = 256: C4's identity pairs).  W3 and W1 are 512 KB each: neither LDS residency nor per-lane L2 fetches serve, so both
// layers' filters are streamed through LDS by LDS-DMA from the layers' stream images (conv_pack.h: pack_chain_stream — the chunk images lie in
// memory in their LDS layout, so every copy is straight).  A block owns 128 rows and has EIGHT waves, two per SIMD: the two waves of a SIMD
// (a pair: waves p and p + 4) own the same 32 rows and split the work by role, so that one's epilogue runs while the other's MFMAs run.
//   * wave A holds the rows' raw fp32 activation fragments, splits them group by group and issues P's MFMAs for a 64-column chunk (two
//     accumulator tiles) in two half-steps of eight channel groups; it deposits the finished sums piece by piece in the pair's two LDS tiles
//     and issues ALL of the block's DMAs, BEHIND its MFMAs of the step (measured: in front of them the matrix pipe stands idle while A issues and B is
//     in its epilogue) — it has no other vector-memory traffic in the loop, so its vmcnt in front of a barrier counts DMAs only;
//   * wave B requests the residual a whole piece ahead, takes a piece of P's sums from the pair's tile, runs chain_piece_p on it (scale / shift,
//     + residual, ReLU, watch, store; y left in the tile), reads y back as fragments, splits and issues Q's MFMAs; it holds Q's sums and runs
//     Q's epilogue at the end.
// Time runs in steps, one block barrier in front of each (34 in all, the same for every wave whatever M is); nothing else synchronises.  In step s
//   A multiplies half s & 1 of chunk s >> 1 from W3 stage (s >> 1) & 1 and deposits piece s - 1 (odd s: tile X; even s: tile Y, from the sums it kept);
//   B works on piece s - 2 (tile X for an even piece, Y for an odd one) with W1 stage (s - 2) % 3;
//   A's DMAs bring half s & 1 of W3's next chunk (into the stage nobody reads) and W1's K step of piece s (into the stage B last read in step s - 1).
// A step's 32 KB are first read in step s + 2: in front of barrier s + 2 A waits with vmcnt(8), which leaves the eight DMAs of step s + 1 in flight
// (vmcnt(0) where a step issued fewer).  A tile is written in one step and read in the next, and the barrier between the two steps is the hand-over.  A pair whose 32 rows lie beyond M skips loads, MFMAs and stores, never a barrier or a DMA.  Per accumulator the
// order is the other forms': channel groups ascending, hi / mid / lo per group, filter fragment first; one running sum per output of Q.
// LDS: W3 2 x 32 KB | W1 3 x 16 KB | tiles 4 pairs x 2 x 4 KB | the scale / shift tables 10 KB = 154 KB.  Nothing crosses blocks.
template <int C, int PARTS>
__global__ __launch_bounds__(512, 1) void k_conv_chain_ring(const ChainArgs ca)
{
    static_assert(C == 256, "the ring's stages hold C = 256's chunk images");
    constexpr int C4 = 4 * C, KT = C / 32, TNP = 2, TNQ = C / 32, NCH = C4 / 64, NPC = 2 * NCH;
    constexpr int WCH = 64 * C * 2;                      // one chunk image of either layer: 64 rows x C channels (W3) = C rows x 64 channels (W1)
    constexpr int WHALF = WCH / 2;                       // four K steps of a W3 chunk image = one K step (a piece's 32 channels) of a W1 chunk image
    constexpr int NW1 = 3;                               // W1's stages: a piece's K step lands two steps ahead of its use
    constexpr int W1_OFF = 2 * WCH, TILE_OFF = W1_OFF + NW1 * WHALF;
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_OFF + 4 * 2 * 32 * 32 * 4];
    __shared__ __attribute__((aligned(16))) float s_tab[2 * C4], s_tabq[2 * C];       // scale | shift of P's and of Q's columns
    const ConvArgs& a = ca.p;
    const ConvArgs& aq = ca.q;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int pair = wave & 3;                           // waves p and p + 4 share a SIMD and 32 rows
    const int l31 = lane & 31, kk = lane >> 5;
    float* const tiles = reinterpret_cast<float*>(smem + TILE_OFF) + pair * (2 * 32 * 32);
    const ChainTile tx{tiles, lane}, ty{tiles + 32 * 32, lane};
    const int swzb = (l31 >> 2) & 3;                     // filter rows in LDS: 16-B chunk c of row r at c ^ ((r >> 2) & 3)
    const int row0 = (blockIdx.x * 4 + pair) * 32;
    const bool live = row0 < a.M;                        // (wave-uniform) a pair without rows keeps the barriers and the DMAs going and does nothing else

    if (wave < 4) {
        // ================================================ wave A: P's sums and the block's DMAs ================================================
        const int t = pair * 64 + lane;
        static_assert(C4 == 4 * 256 && C % 8 == 0 && C / 2 <= 256, "the tables are filled by 256 threads, 16 B each");
        *reinterpret_cast<float4*>(&s_tab[4 * t]) = chain_ld4(a.scale + 4 * t);
        *reinterpret_cast<float4*>(&s_tab[C4 + 4 * t]) = chain_ld4(a.shift + 4 * t);
        if (t < C / 2) *reinterpret_cast<float4*>(&s_tabq[4 * t]) = chain_ld4(t < C / 4 ? aq.scale + 4 * t : aq.shift + 4 * (t - C / 4));      // (read behind the barriers)
        // ---- the DMA: buffer resources over the two images (a lane beyond them would deposit zeros), inline asm as in kernels_conv.hip ----
        typedef unsigned srd_t __attribute__((ext_vector_type(4)));
        srd_t srdP, srdQ;
        {
            const unsigned long long wp = (unsigned long long)(uintptr_t)ca.p_stream, wq = (unsigned long long)(uintptr_t)ca.q_stream;
            srdP[0] = __builtin_amdgcn_readfirstlane((unsigned)wp);
            srdP[1] = __builtin_amdgcn_readfirstlane((unsigned)(wp >> 32) & 0xffffu);
            srdP[2] = (unsigned)(NCH * WCH);
            srdP[3] = 0x00020000u;
            srdQ[0] = __builtin_amdgcn_readfirstlane((unsigned)wq);
            srdQ[1] = __builtin_amdgcn_readfirstlane((unsigned)(wq >> 32) & 0xffffu);
            srdQ[2] = (unsigned)(NCH * WCH);
            srdQ[3] = 0x00020000u;
        }
        const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);
        const unsigned wdst = lds0 + (unsigned)pair * 1024u;           // wave-uniform: lane i's 16 B land at M0 + 16 i; the four A waves copy 4 KB per round
        const unsigned voff = (unsigned)t * 16u;
#define MRCNN_RING_DMA(SRD, SOFF, DST)                                                                         \
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(SRD), "s"(SOFF), "s"(DST) : "memory", "m0");
        // half h (K steps 4 h .. 4 h + 3, 16 KB contiguous) of W3's chunk c -> W3 stage c & 1
        auto fill_w3 = [&](int c, int h) {
            const unsigned src = (unsigned)__builtin_amdgcn_readfirstlane(c) * (unsigned)WCH + (unsigned)(h * WHALF);
            const unsigned dst = wdst + (unsigned)(__builtin_amdgcn_readfirstlane(c) & 1) * (unsigned)WCH + (unsigned)(h * WHALF);
#pragma unroll
            for (int k = 0; k < WHALF / 4096; ++k) MRCNN_RING_DMA(srdP, src + k * 4096u, dst + k * 4096u)
        };
        // W1's K step of piece p (K step p & 1 of chunk p >> 1, 16 KB contiguous) -> W1 stage p % 3
        auto fill_w1 = [&](int p) {
            const unsigned off = (unsigned)(__builtin_amdgcn_readfirstlane(p) & 1) * (unsigned)WHALF;
            const unsigned src = (unsigned)(__builtin_amdgcn_readfirstlane(p) >> 1) * (unsigned)WCH + off;
            const unsigned dst = wdst + (unsigned)W1_OFF + ((unsigned)__builtin_amdgcn_readfirstlane(p) % (unsigned)NW1) * (unsigned)WHALF;
#pragma unroll
            for (int k = 0; k < WHALF / 4096; ++k) MRCNN_RING_DMA(srdQ, src + k * 4096u, dst + k * 4096u)
        };
        fill_w3(0, 0);
        fill_w3(0, 1);
        // step s = 2 c + h: half h of W3's next chunk (first read in step s + 2, its stage last read in step 2 c - 1) and W1's K step of piece s (read in
        // step s + 2, its stage last read in step s - 1): eight DMAs per wave in every step that has a next chunk, four in the last two
        auto ring_step = [&](int c, int h) {
            if (c + 1 < NCH) fill_w3(c + 1, h);
            fill_w1(2 * c + h);
        };
        // this lane's activation fragments (pixel row0 + l31, 16 groups of 16 channels), raw: the three parts do not fit beside a second wave
        // (a row beyond M: zeros)
        uint4 u[2 * KT][2];
        {
            const int m = row0 + l31;
            const float* const src = static_cast<const float*>(a.in) + (long)m * C + 8 * kk;
#pragma unroll
            for (int g = 0; g < 2 * KT; ++g) {
                u[g][0] = u[g][1] = make_uint4(0u, 0u, 0u, 0u);
                if (m < a.M) { u[g][0] = *reinterpret_cast<const uint4*>(src + g * 16); u[g][1] = *reinterpret_cast<const uint4*>(src + g * 16 + 4); }
            }
        }
        f32x16 accP[TNP];
        chain_zero(accP);
        for (int c = 0; c < NCH; ++c) {
            const unsigned char* const w3s = smem + (c & 1) * WCH;     // [K step][64 rows][64 B]
            auto frag_p = [&](uint4 (&b)[TNP], int i) {
#pragma unroll
                for (int j = 0; j < TNP; ++j) b[j] = *reinterpret_cast<const uint4*>(w3s + ((i >> 1) * 64 + j * 32 + l31) * 64 + (((2 * (i & 1) + kk) ^ swzb) << 4));
            };
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // the DMAs of step s - 2 (and, once, everything before the loop) have landed; the eight of step s - 1 stay in flight
                if (2 * c + h == 0 || c + 1 >= NCH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                __syncthreads();                                        // step 2 c + h
                if (!live) { ring_step(c, h); continue; }
                if (h == 0) {
                    if (c > 0) ty.put(accP[1]);                         // the previous chunk's second piece: B left tile Y at the barrier
                    chain_zero(accP);
                }
                // eight groups of 16 channels; group i + 1's filter fragments and parts are formed ahead of group i's MFMAs
                uint4 bv[TNP];
                frag_p(bv, 8 * h);
                ChainParts pt = chain_split<PARTS>(u[8 * h][0], u[8 * h][1]);
#pragma unroll
                for (int i = 8 * h; i < 8 * h + 8; ++i) {
                    uint4 bn[TNP];
                    ChainParts pn;
                    if (i + 1 < 8 * h + 8) { frag_p(bn, i + 1); pn = chain_split<PARTS>(u[i + 1][0], u[i + 1][1]); }
                    chain_mfma_parts<PARTS, TNP>(accP, bv, pt);
                    if (i + 1 < 8 * h + 8) {
#pragma unroll
                        for (int j = 0; j < TNP; ++j) bv[j] = bn[j];
                        pt = pn;
                    }
                }
                ring_step(c, h);                                        // behind the MFMAs: B's MFMAs run beside the DMAs' issue
                if (h == 1) tx.put(accP[0]);                            // the chunk's first piece: B left tile X at the barrier
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                                // step NPC: the last piece's hand-over
        if (live) ty.put(accP[1]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                                // step NPC + 1: B's last piece
#undef MRCNN_RING_DMA
        return;
    }

    // ================================================ wave B: P's epilogue, Q ================================================
    if (!live) {
        for (int s = 0; s < NPC + 2; ++s) __syncthreads();
        return;
    }
    const float* const res = static_cast<const float*>(a.res);
    float* const out = static_cast<float*>(a.out);
    const bool full = row0 + 32 <= a.M;                  // (wave-uniform) no row of the pair lies beyond M
    const ChainRowOffs ro = chain_row_offs(row0, a.M, lane, C4);
    const float* const res0 = res + (long)row0 * C4;     // (wave-uniform) the wave's first row
    float* const out0 = out + (long)row0 * C4;
    const int c4 = (lane & 7) * 4;
    const bool relu = a.act == ACT_RELU;
    bool out_of_range = false, out_of_range_q = false;
    f32x16 accQ[TNQ];
    chain_zero(accQ);
    float4 rv[2][4];                                     // the residual of this piece and of the next
    auto residual = [&](float4 (&r)[4], int p) { chain_residual_piece(r, res0 + p * 32, ro); };
    residual(rv[0], 0);
    __syncthreads();                                     // steps 0 and 1: A's first chunk
    __syncthreads();
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = 2 * c + j;
            residual(rv[j ^ 1], p + 1 < NPC ? p + 1 : p);          // (unconditional: one count of requests in flight on every path; the last is unused)
            __syncthreads();                             // step p + 2: piece p lies in the pair's tile, its K step of W1 in stage j
            const ChainTile& tl = j ? ty : tx;
            const unsigned char* const w1s = smem + W1_OFF + ((unsigned)p % (unsigned)NW1) * WHALF;       // [C rows][64 B]
            // Q's filter fragments of a quarter of a group (two column tiles x 16 channels): quarter h & 3 of group h >> 2
            auto frag_q = [&](uint4 (&b)[TNQ / 4], int h) {
#pragma unroll
                for (int i = 0; i < TNQ / 4; ++i) b[i] = *reinterpret_cast<const uint4*>(w1s + (((h & 3) * (TNQ / 4) + i) * 32 + l31) * 64 + (((2 * (h >> 2) + kk) ^ swzb) << 4));
            };
            uint4 bq[TNQ / 4];
            frag_q(bq, 0);                               // (independent of the epilogue: on its way meanwhile)
            const int n = p * 32 + c4;
            if (full) {
                if (relu) chain_piece_p<true, true>(tl, s_tab, s_tab + C4, rv[j], ro, out0 + p * 32, n, out_of_range);
                else chain_piece_p<true, false>(tl, s_tab, s_tab + C4, rv[j], ro, out0 + p * 32, n, out_of_range);
            } else {
                if (relu) chain_piece_p<false, true>(tl, s_tab, s_tab + C4, rv[j], ro, out0 + p * 32, n, out_of_range);
                else chain_piece_p<false, false>(tl, s_tab, s_tab + C4, rv[j], ro, out0 + p * 32, n, out_of_range);
            }
            // ---- Q: the K step of channels 32 p .. + 31 ----------------------------------------------------------------
            // (per accumulator the order is the other forms': group 0's parts, then group 1's; the quarters only stagger the fragment reads)
            ChainParts pt;
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                if ((h & 3) == 0) pt = tl.template frag<PARTS>(h >> 2);
                uint4 bn[TNQ / 4];
                if (h < 7) frag_q(bn, h + 1);
                __builtin_amdgcn_sched_barrier(0);
                if ((h & 3) == 0) chain_mfma_parts<PARTS, TNQ / 4, TNQ, 0>(accQ, bq, pt);
                else if ((h & 3) == 1) chain_mfma_parts<PARTS, TNQ / 4, TNQ, TNQ / 4>(accQ, bq, pt);
                else if ((h & 3) == 2) chain_mfma_parts<PARTS, TNQ / 4, TNQ, TNQ / 2>(accQ, bq, pt);
                else chain_mfma_parts<PARTS, TNQ / 4, TNQ, 3 * TNQ / 4>(accQ, bq, pt);
                if (h < 7) {
#pragma unroll
                    for (int i = 0; i < TNQ / 4; ++i) bq[i] = bn[i];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // (no barrier follows: A is done with the tiles, a pair without rows is done)
    int lane_q = lane;
    asm volatile("" : "+v"(lane_q));                     // Q's rows are formed here, not carried through the loop (the loop has no register to spare)
    chain_epilogue_q(tx, accQ, s_tabq, s_tabq + C, aq.act == ACT_RELU, chain_rows(row0, a.M, lane_q), static_cast<float*>(aq.out), out_of_range_q);
    if (a.range_flag && out_of_range) atomicOr(a.range_flag, 1);
    if (aq.range_flag && out_of_range_q) atomicOr(aq.range_flag, 1);
}


typedef void (*chain_kernel_t)(const ChainArgs);
template <int PARTS>
static chain_kernel_t chain_kernel(int C, bool sc)
{
    if (C == 256) return k_conv_chain_ring<256, PARTS>;
    if (C == 64) return sc ? k_conv_chain<64, PARTS, true> : k_conv_chain<64, PARTS, false>;
    return sc ? k_conv_chain<128, PARTS, true> : k_conv_chain<128, PARTS, false>;
}

// p / q: the launch arguments of the two layers (conv_dispatch.hip has checked the pair: conv_chain_fusable); parts 2 | 3
// the form follows from C = q.Cout: 64 — LDS-resident and persistent (a 64-channel shortcut or none; n_cus sizes its grid), 128 — filters from L2,
// 256 — the ring (identity pairs only, from p_stream / q_stream: the layers' stream images)
void conv_chain_launch(hipStream_t s, const ConvArgs& p, const ConvArgs& q, int parts, int n_cus, const void* p_stream, const void* q_stream)
{
    ChainArgs ca{p, q, p_stream, q_stream};
    const bool sc = p.sc_in != nullptr;
    const int C = q.Cout;
    dim3 grid((p.M + 127) / 128), block(C == 256 ? 512 : 256);
    MRCNN_REQUIRE((C == 64 || C == 128 || C == 256) && (parts == 2 || parts == 3), MRCNN_ERR_INVALID, "conv_chain_launch: C %d, %d parts", C, parts);
    if (C == 256) MRCNN_REQUIRE(!sc && p.res && p_stream && q_stream, MRCNN_ERR_INVALID, "conv_chain_launch: C = 256 runs identity pairs from their stream images");
    if (C == 64) {
        MRCNN_REQUIRE((!sc || p.sc_Cin == 64) && n_cus > 0, MRCNN_ERR_INVALID, "conv_chain_launch: the LDS-resident form holds C = 64's filters");
        const int tiles256 = (p.M + 255) / 256;
        grid = dim3(tiles256 < n_cus ? tiles256 : n_cus); block = dim3(512);
    }
    hipLaunchKernelGGL(parts == 3 ? chain_kernel<3>(C, sc) : chain_kernel<2>(C, sc), grid, block, 0, s, ca);
}

}  // namespace mrcnn
