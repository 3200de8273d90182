// kernels_conv.hip — the convolution family of the trunk and heads on gfx950 matrix cores: the implicit-GEMM kernel
// and its launches.  (Which kernel of the family runs a layer: conv_dispatch.hip; the small element-wise kernels
// around the convolutions: kernels_elementwise.hip.)
//
// Replaces the built-in Core ML layers of MaskRCNN.mlmodel / Classifier.mlmodel / Mask.mlmodel
// (spec emitted by Sources/maskrcnn/Python/Conversion/task.py:69-116 of the reference): 7×7/3×3/1×1
// convolutions with folded BatchNorm, ReLU, residual adds, FPN nearest-neighbour upsample+add, the
// RPN / box / mask heads (inner products as 1×1 convolutions, the 2×2 stride-2 transposed
// convolution as a scatter GEMM), soft-max and sigmoid.
//
// Kernel design (fp32: exact f32 MFMA `v_mfma_f32_32x32x2_f32`; fp16: `v_mfma_f32_32x32x16_f16`):
//   implicit GEMM  out[m][n] = Σ_k A[m][k]·Wt[n][k],  m = (image, oh, ow), k = (tap, cin), n = cout
//   * activations NHWC and filters packed [cout][tap][cin], so BOTH operands are "rows of K":
//     every global load is a 16-B piece of a 128-B contiguous run (32 fp32 / 64 fp16 channels of one tap);
//   * 128×BN block tile, K tile of 128 B, 8 waves (wave64) as 4×2, each wave a (TM×32)×(TN×32) sub-tile
//     of 32×32 MFMA accumulators; K is permuted inside the tile (lane kk∈{0,1} owns one 16-B chunk of
//     every 32-B pair) so a lane fetches its operands for four fp32 MFMA steps / one fp16 MFMA with ONE
//     ds_read_b128 — identical permutation on both operands, so the sum is unchanged;
//   * operands go global→LDS by DMA into two XOR-swizzled buffers (details at the kernel below);
//   * fused epilogue: per-channel scale/shift (folded BN + bias), residual (optionally read at
//     (oh>>1, ow>>1): FPN top-down upsample+add), ReLU / sigmoid, optional column split into two
//     outputs (RPN class + bbox from one GEMM) or 2×2 scatter (transposed conv);
//   * XCD-aware block→tile map: the 8 XCDs get contiguous runs of tiles, N-tiles of one M-tile
//     adjacent, so an A tile is fetched into one XCD's L2 once.
#include "conv_device.h"

namespace mrcnn {

// ------------------------------------------------------------------------------------------------
// The implicit-GEMM kernel.  T = float   : v_mfma_f32_32x32x2_f32  (exact fp32, 157.3 TFLOP/s peak), K tile = 32
//                            T = _Float16: v_mfma_f32_32x32x16_f16 (fp32 accumulate, ~2.5 PFLOP/s peak), K tile = 64
// Operands are staged global→LDS directly (global_load_lds_dwordx4): no VGPR round trip, no ds_write,
// no address/register traffic between the loads and the MFMAs — a register-staged loop (round-1
// history) lost 13 % (fp32) / 40 % (fp16) of the MFMA rate to that path even with
// cache-hot loads.
//   * LDS rows are unpadded 128-B K runs (the DMA writes wave-uniform base + lane×16, so rows cannot
//     be padded); bank conflicts are removed by an XOR swizzle instead: 16-B chunk c of row r lives
//     at chunk position c ^ ((r >> 1) & 7).  The permutation is applied to the per-lane SOURCE
//     address (inside one 128-B line, so coalescing is unchanged) and to the ds_read address.
//     For ds_read_b128's 16-lane groups the pairs (r & 1, (r >> 1) & 7) are all distinct → conflict-free.
//   * the DMAs go through buffer resources (buffer_load_dwordx4 … lds): out-of-image taps (zero padding) and rows beyond
//     M carry an out-of-range offset and the hardware deposits zeros — not predicated, no memory access.
//   * two LDS buffers: the DMA of tile k+1 is issued right after the barrier that retired buffer
//     (k+1)&1 and lands while tile k is being multiplied; one vmcnt(0) + barrier per K step.
// ------------------------------------------------------------------------------------------------
template <typename T, typename TW, int BN, int TM, int TN, int WM, int WN, int STAGES, int PARTS = 2>
__global__ __launch_bounds__(WM * WN * 64, WM * WN >= 8 ? 4 : 2) void k_conv_mfma_glds(const ConvArgs a)     // two blocks per CU
{
    // SPLIT: fp32 activations × fp16 filters as PARTS (2 or 3) fp16 MFMA passes over a split of the activations
    constexpr bool SPLIT = sizeof(T) == 4 && sizeof(TW) == 2;
    static_assert(PARTS == 2 || PARTS == 3, "split parts");
    static_assert(sizeof(T) == sizeof(TW) || SPLIT, "operand types");
    constexpr int BM = WM * TM * 32;
    static_assert(WN * TN * 32 == BN, "tile shape");
    constexpr int EPV = Elem<T>::EPV;
    constexpr int BK = 8 * EPV;
    constexpr int NT = WM * WN * 64;
    constexpr int RPT = NT / 8;
    constexpr int AP = BM / RPT;
    constexpr int BP = SPLIT ? (BN * 4 > NT ? BN * 4 / NT : 1) : BN / RPT;   // SPLIT: 64-B filter rows, 16 B per thread and DMA
    static_assert(AP >= 1 && BP >= 1 && AP <= 4 && BP <= 4 && RPT % 16 == 0, "staging shape");
    static_assert(!SPLIT || BP <= 2, "split mode: the filter tile is staged by at most two DMAs per thread");
    constexpr int ROWB = 128;
    constexpr int BROWB = SPLIT ? 64 : 128;                     // bytes of one filter row per K step
    constexpr int A_STAGE = BM * ROWB, B_STAGE = BN * BROWB;
    constexpr int CPASS = BM * BN * 4 > 64 * 1024 ? WN : 1;    // column passes of the epilogue (fp32 C tile of at most 64 KB)
    constexpr int C_BYTES = BM * (BN / CPASS + 4) * 4;         // rows padded by 16 B (conv_epilogue)
    static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
    constexpr int NLOADS = SPLIT ? AP : AP + BP;                // DMA instructions per tile per thread (SPLIT: waves past BN/16 issue no filter DMA)
    constexpr int SMEM_OPS = STAGES * (A_STAGE + B_STAGE);      // ring of operand buffers
    // fp16 tensors, 32 x 64 wave tiles: the wave-private epilogue stages 32 x 68 floats per wave (conv_epilogue_wave_h)
    constexpr bool WAVE_H = sizeof(T) == 2 && TN == 2 && BN == 128 && CPASS == 1;
    constexpr int WAVE_H_BYTES = WAVE_H ? WM * WN * 32 * 68 * 4 : 0;
    constexpr int SMEM_ = SMEM_OPS > C_BYTES ? SMEM_OPS : C_BYTES;
    constexpr int SMEM = SMEM_ > WAVE_H_BYTES ? SMEM_ : WAVE_H_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    constexpr bool DIRECT_OK = CPASS == 1 && BN >= 64;                 // (the 32-wide tiles fill the LDS of two blocks to the byte)
    __shared__ __attribute__((aligned(16))) float s_tab[DIRECT_OK ? 2 * BN : 4];       // scale | shift of the block's columns (direct epilogue)
    const T* const in = static_cast<const T*>(a.in);
    const TW* const wgt = static_cast<const TW*>(a.wgt);
#ifdef MRCNN_CONV_ABLATE
    // experiment: de-phase the two blocks of a CU once, at the start of the launch (blocks 256..511 take the second slots)
    if ((a.dbg >> 16) && blockIdx.x >= 256 && blockIdx.x < 512) {
        const unsigned long long t0 = wall_clock64();
        while (wall_clock64() - t0 < (unsigned long long)(a.dbg >> 16)) __builtin_amdgcn_s_sleep(16);      // units of 10 ns
    }
#endif

    // KCH: the kernel carries the canonical K chunks of long-K 1x1 layers (ConvArgs::kchunks; conv_k_chunks below).  The 8-wave
    // 128-column instantiation has no room for the second accumulator set (112 of the 128 VGPRs that four waves per SIMD
    // allow): chunked layers take the 4-wave 128-column form instead (conv_forward; same speed on them, gpurun_out/r4v)
    constexpr bool KCH = SPLIT && !(BN == 128 && WM * WN >= 8);
    const int ksplit = KCH ? a.ksplit : 1;
    const int nblocks = a.tiles_m * a.tiles_n * ksplit;
    const int bid = blockIdx.x;
    const int q = nblocks >> 3, r8 = nblocks & 7;
    const int xcd = bid & 7, local = bid >> 3;
    const int unit = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + local;
    const int tile = unit / ksplit, chunk = unit - tile * ksplit;          // the blocks of a tile are neighbours in the walk (mostly one XCD)
    const int mt = tile / a.tiles_n, nt = tile - mt * a.tiles_n;
    const int m0 = mt * BM, n0 = nt * BN;

    const int t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63;
    const int r0 = t >> 3;                              // row inside a staging pass
    const int kq = (t & 7) ^ ((r0 >> 1) & 7);           // SOURCE chunk held at LDS chunk position (t & 7)

    // Both operands are addressed through buffer resources (raw, stride 0): 32-bit byte offsets per lane, and a lane
    // whose offset lies beyond the resource deposits ZEROS in LDS — zero padding and rows beyond M cost no memory access
    // and no zero page.  (Also the fastest form of the DMA on this chip: +5-8 % over 64-bit lane addresses in the kernel,
    // tools/probes/dma_probe.hip.)  The activation resource starts at the first image the block touches, so that offsets
    // stay small whatever the batch, and ends with the tensor.
    const int ohw = a.OH * a.OW;
    const int b0 = m0 / ohw;
    constexpr unsigned OOB = 0xffffff00u;
    typedef unsigned srd_t __attribute__((ext_vector_type(4)));
    srd_t srdA, srdB;
    {
        const unsigned long long ia = (unsigned long long)(uintptr_t)(in + (long)b0 * a.in_sB), wa = (unsigned long long)(uintptr_t)wgt;
        const unsigned long long rest = (unsigned long long)(a.M / ohw - b0) * (unsigned long long)a.in_sB * sizeof(T);
        srdA[0] = __builtin_amdgcn_readfirstlane((unsigned)ia);
        srdA[1] = __builtin_amdgcn_readfirstlane((unsigned)(ia >> 32) & 0xffffu);
        srdA[2] = __builtin_amdgcn_readfirstlane((unsigned)(rest < OOB ? rest : OOB));
        srdA[3] = 0x00020000u;
        srdB[0] = __builtin_amdgcn_readfirstlane((unsigned)wa);
        srdB[1] = __builtin_amdgcn_readfirstlane((unsigned)(wa >> 32) & 0xffffu);
        srdB[2] = 0xffffffffu;
        srdB[3] = 0x00020000u;
    }
    // SC (fused shortcut, round 4): behind the layer's own K steps the SAME loop runs the K steps of the block's shortcut convolution — a
    // second 1x1 over the block's input (other tensor, strides, filters, K).  The DMA stream switches source when the layer's channels are
    // exhausted (the ring never drains: no second pipeline fill), the accumulators change hands at that step (`tot` keeps the layer's sums,
    // `acc` restarts for the shortcut's), and the epilogue forms the residual y_sc = acc * scale2 + shift2 where it would have loaded it.
    const bool sc_fused = KCH && DIRECT_OK && a.sc_in != nullptr;
    unsigned a_ob[AP];          // byte offset of tap (0, 0) of the staged row from the resource base (mod 2^32: it may lie before it)
    unsigned a_ob2[KCH ? AP : 1];                         // ... of the shortcut's input row
    int ih0[AP], iw0[AP];
    bool a_ok[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        const int m = m0 + r0 + RPT * p;
        a_ok[p] = m < a.M;
        const int mm = a_ok[p] ? m : 0;
        const int b = mm / ohw, rem = mm - b * ohw;
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        ih0[p] = oh * a.stride - a.padH;
        iw0[p] = ow * a.stride - a.padW;
        a_ob[p] = (unsigned)(((long)(b - b0) * a.in_sB + (long)ih0[p] * a.in_sH + (long)iw0[p] * a.in_sW + kq * EPV) * (long)sizeof(T));
        if constexpr (KCH)
            a_ob2[p] = (unsigned)(((long)(b - b0) * a.sc_in_sB + (long)(oh * a.sc_stride) * a.sc_in_sH + (long)(ow * a.sc_stride) * a.sc_in_sW + kq * EPV) * (long)sizeof(T));
    }
    srd_t srdA2 = srdA, srdB2 = srdB;
    if constexpr (KCH) {
        if (sc_fused) {
            const unsigned long long ia = (unsigned long long)(uintptr_t)(static_cast<const T*>(a.sc_in) + (long)b0 * a.sc_in_sB), wa = (unsigned long long)(uintptr_t)a.sc_wgt;
            const unsigned long long rest = (unsigned long long)(a.M / ohw - b0) * (unsigned long long)a.sc_in_sB * sizeof(T);
            srdA2[0] = __builtin_amdgcn_readfirstlane((unsigned)ia);
            srdA2[1] = __builtin_amdgcn_readfirstlane((unsigned)(ia >> 32) & 0xffffu);
            srdA2[2] = __builtin_amdgcn_readfirstlane((unsigned)(rest < OOB ? rest : OOB));
            srdB2[0] = __builtin_amdgcn_readfirstlane((unsigned)wa);
            srdB2[1] = __builtin_amdgcn_readfirstlane((unsigned)(wa >> 32) & 0xffffu);
        }
    }
    int cin_tiles = a.Cin / BK;
    const int KT_main = a.KH * a.KW * cin_tiles;
    const int KT_all = KT_main + (sc_fused ? a.sc_Cin / BK : 0);
    const int KT = KT_all / ksplit;                       // K steps of THIS block: one chunk when the tile is shared
    const int kbeg = chunk * KT;
    // wave-uniform LDS destinations: this wave's 8 rows of each staging pass
    const int wrow = __builtin_amdgcn_readfirstlane(wave) * 8;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(
        (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);   // LDS byte address of smem

    // ---- DMA address generation, kept off the per-tile critical path ------------------------------
    // A (activations): one 32-bit byte offset per staged row, advanced by a per-row step each tile
    //   (step = one K tile, or 0 when the tap falls outside the image and the row's offset is out of range → zeros);
    //   the bounds test and the select run only when the TAP changes (every Cin/BK tiles).
    // B (filters): scalar offset (advanced by one K tile) + loop-invariant 32-bit per-lane byte offset.
    // The DMA itself goes through inline asm on purpose: with the builtin hipcc treats it as an LDS
    // store it must order against every later ds_read and drains it with vmcnt(0) at the top of the
    // step, which makes the copy synchronous.  In asm the compiler does not count it, so the waits
    // are placed by hand (M0 = wave-uniform LDS byte address; lane i's 16 B land at M0 + 16 i).
    static_assert(AP <= 4 && BP <= 4, "per-row DMA state is spelled out for <= 4 A rows / <= 4 B rows");
    unsigned oa0 = OOB, oa1 = OOB, oa2 = OOB, oa3 = OOB;
    unsigned sa0 = 0, sa1 = 0, sa2 = 0, sa3 = 0;
    // SPLIT: thread t stages 16 B (8 fp16 channels) of filter row t>>2; chunk c of row r sits at position c ^ ((r>>2)&3)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const bool wave_has_b = !SPLIT || BN * 4 >= NT || wave_u < BN / 16;
    unsigned vb0 = SPLIT ? (unsigned)(((size_t)(t >> 2) * a.Ktot + (((t & 3) ^ ((t >> 4) & 3)) << 3)) * sizeof(TW))
                               : (unsigned)(((size_t)r0 * a.Ktot + kq * EPV) * sizeof(T));
    unsigned vb1 = SPLIT ? vb0 + (unsigned)((size_t)(NT / 4) * a.Ktot * sizeof(TW))
                               : (unsigned)(((size_t)(r0 + RPT) * a.Ktot + kq * EPV) * sizeof(T));
    const unsigned vb2 = (unsigned)(((size_t)(r0 + 2 * RPT) * a.Ktot + kq * EPV) * sizeof(T));
    const unsigned vb3 = (unsigned)(((size_t)(r0 + 3 * RPT) * a.Ktot + kq * EPV) * sizeof(T));
    unsigned sob = (unsigned)((size_t)n0 * a.Ktot * sizeof(TW));      // uniform: byte offset of the K tile in the filter
    int kh = 0, kw = 0, ct = 0;
#define MRCNN_SET_TAP(P)                                                                                       \
    if constexpr (AP > P) {                                                                                    \
        const int ih = ih0[P] + kh, iw = iw0[P] + kw;                                                          \
        const bool ok = a_ok[P] && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;               \
        oa##P = ok ? a_ob[P] + (unsigned)(((long)kh * a.in_sH + (long)kw * a.in_sW) * (long)sizeof(T)) : OOB;  \
        sa##P = ok ? BK * (unsigned)sizeof(T) : 0u;                                                            \
    }
    bool sc_pending = sc_fused;
    /* the layer's channels are exhausted: the stream continues with the shortcut's input and filters (1x1, no padding: every staged row in range) */
#define MRCNN_SC_ROW(P) if constexpr (AP > P) { oa##P = a_ok[P] ? a_ob2[P] : OOB; sa##P = a_ok[P] ? BK * (unsigned)sizeof(T) : 0u; }
#define MRCNN_SC_SWITCH()                                                                                      \
    {                                                                                                          \
        if constexpr (KCH) {                                                                                   \
            sc_pending = false;                                                                                \
            MRCNN_SC_ROW(0) MRCNN_SC_ROW(1) MRCNN_SC_ROW(2) MRCNN_SC_ROW(3)                                    \
            srdA = srdA2; srdB = srdB2;                                                                        \
            cin_tiles = a.sc_Cin / BK;                                                                         \
            vb0 = (unsigned)(((size_t)(t >> 2) * a.sc_Cin + (((t & 3) ^ ((t >> 4) & 3)) << 3)) * sizeof(TW));   \
            vb1 = vb0 + (unsigned)((size_t)(NT / 4) * a.sc_Cin * sizeof(TW));                                  \
            sob = (unsigned)((size_t)n0 * a.sc_Cin * sizeof(TW));                                              \
        }                                                                                                      \
    }
#define MRCNN_GLDS_V(VOFF, DST)                                                                                \
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(VOFF), "s"(srdA), "s"(DST) : "memory", "m0");
#define MRCNN_GLDS_S(VOFF, SOFF, DST)                                                                          \
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(VOFF), "s"(srdB), "s"(SOFF), "s"(DST) : "memory", "m0");
#define MRCNN_DMA_A(P) if constexpr (AP > P) { MRCNN_GLDS_V(oa##P, da + P * RPT * ROWB); oa##P += sa##P; }
#define MRCNN_DMA_TILE(KT_, BUF_)                                                                              \
    {                                                                                                          \
        const unsigned da = lds0 + (BUF_) * A_STAGE + wrow * ROWB;                                             \
        const unsigned db = lds0 + STAGES * A_STAGE + (BUF_) * B_STAGE + (SPLIT ? wave_u * 1024 : wrow * ROWB); \
        MRCNN_DMA_A(0) MRCNN_DMA_A(1) MRCNN_DMA_A(2) MRCNN_DMA_A(3)                                            \
        if (wave_has_b) MRCNN_GLDS_S(vb0, sob, db);                                                            \
        if constexpr (BP > 1) MRCNN_GLDS_S(vb1, sob, db + (SPLIT ? NT * 16 : RPT * ROWB));                     \
        if constexpr (BP > 2) MRCNN_GLDS_S(vb2, sob, db + 2 * RPT * ROWB);                                     \
        if constexpr (BP > 3) MRCNN_GLDS_S(vb3, sob, db + 3 * RPT * ROWB);                                     \
        sob += BK * (unsigned)sizeof(TW);                                                                      \
        if (++ct == cin_tiles) {                                                                               \
            ct = 0;                                                                                            \
            if (KCH && sc_pending) { MRCNN_SC_SWITCH() }                                                       \
            else {                                                                                             \
                if (++kw == a.KW) { kw = 0; ++kh; }                                                            \
                MRCNN_SET_TAP(0) MRCNN_SET_TAP(1) MRCNN_SET_TAP(2) MRCNN_SET_TAP(3)                            \
            }                                                                                                  \
        }                                                                                                      \
    }
    MRCNN_SET_TAP(0) MRCNN_SET_TAP(1) MRCNN_SET_TAP(2) MRCNN_SET_TAP(3)
    if constexpr (KCH) {
        if (kbeg) {                                       // (1x1 layers only: a K step is a channel step)
            oa0 += kbeg * sa0; oa1 += kbeg * sa1; oa2 += kbeg * sa2; oa3 += kbeg * sa3;
            sob += (unsigned)kbeg * BK * (unsigned)sizeof(TW);
        }
    }

    const int wm = wave / WN, wn = wave - wm * WN;
    const int l31 = lane & 31, kk = lane >> 5;
    const int swz = (l31 >> 1) & 7;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    // canonical K chunks, one block per tile: `tot` folds the finished chunks, `acc` restarts from zero at every boundary
    f32x16 tot[KCH ? TM : 1][KCH ? TN : 1];
    const int klen = KCH ? KT_all / a.kchunks : 0;
    int kb = (KCH && a.kchunks > 1 && ksplit == 1) ? klen : (sc_fused ? KT_main : 0x7fffffff);        // (fused shortcut: the accumulators change hands behind the layer's own steps)
    if constexpr (KCH) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) tot[i][j][e] = 0.0f;
    }
#define MRCNN_KFOLD                                                                                            \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                             \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                         \
            _Pragma("unroll") for (int e = 0; e < 16; ++e) { tot[i][j][e] += acc[i][j][e]; acc[i][j][e] = 0.0f; }

    // Ring of STAGES operand buffers, STAGES-1 tiles in flight: tile k+STAGES-1 is issued at the top of
    // step k, and only tile k+1 has to have landed at the end of it — counted vmcnt lets the
    // NLOADS·(STAGES-2) most recent DMAs stay outstanding across the barrier.  STAGES = 2 for the
    // 128-wide tile (a step is 2048 MFMA cycles per wave, longer than the DMA latency); the narrow
    // tiles run on under-filled grids with short steps and use deeper rings.
    // direct epilogue (conv_device.h): its scale / shift table goes to LDS before the first barrier
    const bool direct = DIRECT_OK && a.direct;
    if (direct && t < BN / 2) {
        const int c = (t < BN / 4 ? t : t - BN / 4) * 4;
        const float* src = t < BN / 4 ? a.scale : a.shift;
        const float fill = t < BN / 4 ? 1.0f : 0.0f;
        *reinterpret_cast<float4*>(&s_tab[(t < BN / 4 ? 0 : BN) + c]) =
            src ? *reinterpret_cast<const float4*>(src + n0 + c) : make_float4(fill, fill, fill, fill);
    }
    __shared__ __attribute__((aligned(16))) float s_tab2[KCH && DIRECT_OK ? 2 * BN : 4];       // scale | shift of the shortcut convolution's columns
    if constexpr (KCH && DIRECT_OK) {
        if (sc_fused && t < BN / 2) {
            const int c = (t < BN / 4 ? t : t - BN / 4) * 4;
            const float* src = t < BN / 4 ? a.sc_scale : a.sc_shift;
            const float fill = t < BN / 4 ? 1.0f : 0.0f;
            *reinterpret_cast<float4*>(&s_tab2[(t < BN / 4 ? 0 : BN) + c]) =
                src ? *reinterpret_cast<const float4*>(src + n0 + c) : make_float4(fill, fill, fill, fill);
        }
    }
    MRCNN_DMA_TILE(0, 0)
    if (STAGES > 2 && KT > 1) MRCNN_DMA_TILE(1, 1)
    if (STAGES > 3 && KT > 2) MRCNN_DMA_TILE(2, 2)
    if (KT - 1 >= STAGES - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLOADS * (STAGES - 2)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();          // tile 0 is in LDS

    // One K step on buffer BUF; the DMA of tile KTV + STAGES - 1 goes to buffer NBUF (the one retired
    // by the previous step's barrier).  BUF / NBUF are compile-time constants (loop unrolled by
    // STAGES), so every LDS offset folds into an instruction immediate and the four swizzled lane
    // addresses are loop-invariant.
    const unsigned char* const la = smem + (wm * TM * 32 + l31) * ROWB;
    const unsigned char* const lb = smem + STAGES * A_STAGE + (wn * TN * 32 + l31) * BROWB;
    const int co0 = ((0 + kk) ^ swz) << 4, co1 = ((2 + kk) ^ swz) << 4, co2 = ((4 + kk) ^ swz) << 4, co3 = ((6 + kk) ^ swz) << 4;
    // Operand fetch for the four 32-B K groups of a step is issued up front, ahead of the first MFMA:
    // LDS returns in order, so the waits count down (lgkmcnt) and the reads of group g+1.. are in
    // flight under the MFMAs of group g — needed when a SIMD holds a single wave (narrow tiles on
    // under-filled grids), free otherwise.
    // SPLIT: a step is 32 channels = two fp16 MFMA K groups; lane kk of group g owns channels
    // [8(2g+kk), +8): two fp32 chunks of the activation row, one fp16 chunk of the filter row.
    const int swzb = (l31 >> 2) & 3;
    const int cb0 = ((0 + kk) ^ swzb) << 4, cb1 = ((2 + kk) ^ swzb) << 4;
    const int ca0 = ((0 + 2 * kk) ^ swz) << 4, ca1 = ((1 + 2 * kk) ^ swz) << 4, ca2 = ((4 + 2 * kk) ^ swz) << 4, ca3 = ((5 + 2 * kk) ^ swz) << 4;
#define MRCNN_KLOAD(G, BUF, CO)                                                                                \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) av[G][i] = *reinterpret_cast<const uint4*>(la + (BUF) * A_STAGE + i * 32 * ROWB + (CO)); \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) bv[G][j] = *reinterpret_cast<const uint4*>(lb + (BUF) * B_STAGE + j * 32 * ROWB + (CO));
#define MRCNN_KLOAD_SPLIT(G, BUF, CA, CA1, CB)                                                                 \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                           \
        av[2 * G][i] = *reinterpret_cast<const uint4*>(la + (BUF) * A_STAGE + i * 32 * ROWB + (CA));           \
        av[2 * G + 1][i] = *reinterpret_cast<const uint4*>(la + (BUF) * A_STAGE + i * 32 * ROWB + (CA1));      \
    }                                                                                                          \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) bv[G][j] = *reinterpret_cast<const uint4*>(lb + (BUF) * B_STAGE + j * 32 * BROWB + (CB));
#define MRCNN_KMATH(G)                                                                                         \
    {                                                                                                          \
        if constexpr (sizeof(T) == 4) {                                                                        \
            _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                      \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                 \
                    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                           \
                        const uint32_t au = c == 0 ? av[G][i].x : c == 1 ? av[G][i].y : c == 2 ? av[G][i].z : av[G][i].w;  \
                        const uint32_t bu = c == 0 ? bv[G][j].x : c == 1 ? bv[G][j].y : c == 2 ? bv[G][j].z : bv[G][j].w;  \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(bu), __uint_as_float(au), acc[i][j], 0, 0, 0); \
                    }                                                                                          \
        } else {                                                                                               \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                 \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[G][j]),    \
                                                                       __builtin_bit_cast(f16x8, av[G][i]), acc[i][j], 0, 0, 0); \
        }                                                                                                      \
    }
#define MRCNN_KMATH_SPLIT(G)                                                                                   \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                           \
        f16x8 hi, lo, lo2;                                                                                     \
        if constexpr (PARTS == 3) split_hi_mid_lo(av[2 * G][i], av[2 * G + 1][i], hi, lo, lo2);                \
        else split_hi_lo(av[2 * G][i], av[2 * G + 1][i], hi, lo);                                              \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                         \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[G][j]), hi, acc[i][j], 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                         \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[G][j]), lo, acc[i][j], 0, 0, 0); \
        if constexpr (PARTS == 3) {                                                                            \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bv[G][j]), lo2, acc[i][j], 0, 0, 0); \
        }                                                                                                      \
    }
#ifdef MRCNN_CONV_ABLATE      /* measurement build (make ablate): a.dbg 256 no MFMAs (split modes), 512 no DMA in the main loop, 1024 no epilogue, 2048 no residual, 4096 no stores */
#define MRCNN_ABL_NODMA && !(a.dbg & 512)
#define MRCNN_ABL_IFMMA if (!(a.dbg & 256))
#else
#define MRCNN_ABL_NODMA
#define MRCNN_ABL_IFMMA
#endif
#define MRCNN_STEP(BUF, NBUF, KTV)                                                                             \
    {                                                                                                          \
        const bool more = (KTV) + STAGES - 1 < KT MRCNN_ABL_NODMA;                                             \
        if (more) MRCNN_DMA_TILE((KTV) + STAGES - 1, NBUF)                                                     \
        if constexpr (KCH) { if ((KTV) == kb) { MRCNN_KFOLD kb += klen; } }                                    \
        uint4 av[4][TM], bv[4][TN];                                                                            \
        if constexpr (SPLIT) {                                                                                 \
            MRCNN_KLOAD_SPLIT(0, BUF, ca0, ca1, cb0) MRCNN_KLOAD_SPLIT(1, BUF, ca2, ca3, cb1)                  \
            if constexpr (BN < 128) __builtin_amdgcn_sched_barrier(0);                                         \
            MRCNN_ABL_IFMMA { MRCNN_KMATH_SPLIT(0) MRCNN_KMATH_SPLIT(1) }                                      \
        } else {                                                                                               \
            MRCNN_KLOAD(0, BUF, co0) MRCNN_KLOAD(1, BUF, co1) MRCNN_KLOAD(2, BUF, co2) MRCNN_KLOAD(3, BUF, co3) \
            if constexpr (BN < 128) __builtin_amdgcn_sched_barrier(0); /* keep the reads ahead of the MFMAs */ \
            MRCNN_KMATH(0) MRCNN_KMATH(1) MRCNN_KMATH(2) MRCNN_KMATH(3)                                        \
        }                                                                                                      \
        /* tile KTV+1 must have landed before the barrier hands its buffer over */                             \
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLOADS * (STAGES - 2)) : "memory");                 \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
        __syncthreads(); /* ... and every wave is done reading BUF */                                          \
    }
    for (int kt = 0; kt < KT; kt += STAGES) {
        MRCNN_STEP(0, STAGES - 1, kt)
        if (kt + 1 < KT) MRCNN_STEP(1, 0, kt + 1)
        if constexpr (STAGES > 2) { if (kt + 2 < KT) MRCNN_STEP(2, 1, kt + 2) }
        if constexpr (STAGES > 3) { if (kt + 3 < KT) MRCNN_STEP(3, 2, kt + 3) }
    }
    if constexpr (KCH) {
        if (ksplit > 1) {
            // this block's chunk goes to the scratch (16-B piece q of thread t at [tile][chunk][q][t]: full lines); the block that
            // arrives last — whichever it is — folds the chunks in THE canonical order and runs the epilogue.  The blocks of a tile
            // may sit on different XCDs (one L2 each): the partial sums are stored and loaded at DEVICE scope (sc1: written through /
            // fetched past the non-coherent L2 lines), the stores have completed (vmcnt) before the block counts itself in, and the
            // counter is a device-scope atomic — no cache-wide write-back or invalidate, which is what a __threadfence() costs here
            // (measured: 18.6 -> 86 us on C4's branch2a at batch 1, gpurun_out/r4w).  The counter is left at zero for the next launch.
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            constexpr int NP = TM * TN * 4;                        // 16-B pieces of a thread's accumulators
            constexpr int SC1 = 16;                                // cache policy of the buffer builtins: device scope
            float* const tbase = a.ks_scratch + (size_t)tile * ksplit * NP * NT * 4;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(tbase, 0, 0x7fffffff, 0x00020000);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        typedef float f32x4 __attribute__((ext_vector_type(4)));
                        const f32x4 v = {acc[i][j][4 * qd], acc[i][j][4 * qd + 1], acc[i][j][4 * qd + 2], acc[i][j][4 * qd + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, ((chunk * NP + (i * TN + j) * 4 + qd) * NT + t) * 16, 0, SC1);
                    }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __shared__ unsigned s_arrived;
            __syncthreads();                                       // every thread's stores have completed
            if (t == 0) s_arrived = __hip_atomic_fetch_add(a.ks_count + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (s_arrived != (unsigned)(ksplit - 1)) return;
            if (t == 0) __hip_atomic_store(a.ks_count + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
            u32x4 cur[NP], nxt[NP];
#pragma unroll
            for (int u = 0; u < NP; ++u) cur[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * NT + t) * 16, 0, SC1);
            for (int c = 0; c < ksplit; ++c) {
                if (c + 1 < ksplit) {
#pragma unroll
                    for (int u = 0; u < NP; ++u) nxt[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (((c + 1) * NP + u) * NT + t) * 16, 0, SC1);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[i][j][4 * qd + e] += __uint_as_float(cur[(i * TN + j) * 4 + qd][e]);
#pragma unroll
                for (int u = 0; u < NP; ++u) cur[u] = nxt[u];
            }
        } else if (a.kchunks > 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = tot[i][j][e] + acc[i][j][e];
        }
    }
#undef MRCNN_KFOLD
#undef MRCNN_STEP
#undef MRCNN_KMATH_SPLIT
#undef MRCNN_KMATH
#undef MRCNN_KLOAD_SPLIT
#undef MRCNN_KLOAD
#undef MRCNN_DMA_TILE
#undef MRCNN_DMA_A
#undef MRCNN_SC_SWITCH
#undef MRCNN_SC_ROW
#undef MRCNN_GLDS_V
#undef MRCNN_GLDS_S
#undef MRCNN_SET_TAP
#ifdef MRCNN_CONV_ABLATE
    if (a.dbg & 1024) { if (a.dbg == 12345678) static_cast<float*>(a.out)[t] = acc[0][0][0]; return; }
#endif
    if constexpr (DIRECT_OK) {
        if (direct && a.sel_partial) {           // selected-class mode, wave-private form (conv_forward sets direct for it only with 64-column parts)
            if constexpr (BN == 128 && TM == 1 && TN == 2) conv_epilogue_sel_wave<T, BN, TM, TN>(a, acc, s_tab, m0 + wm * TM * 32, n0, wn * TN * 32, lane);
            return;
        }
        if (direct) {
            if constexpr (sizeof(T) == 4) {
                // fp32 tensors (a.direct == 2): through a wave-private 32 x 36-float LDS tile (the operand ring is free: the K loop
                // ended in a barrier) — full-line stores without the two block barriers of the staged epilogue
                static_assert(WM * WN * 32 * 36 * 4 <= SMEM, "wave-private epilogue tiles fit in the operand ring");
                if constexpr (KCH) {
                    if (sc_fused) {           // the layer's sums wait in `tot`, the shortcut's are in `acc`
                        conv_epilogue_wave<BN, TM, TN>(a, tot, reinterpret_cast<float*>(smem) + wave * (32 * 36), s_tab, m0 + wm * TM * 32, n0, wn * TN * 32, lane, acc, s_tab2);
                        return;
                    }
                }
                conv_epilogue_wave<BN, TM, TN>(a, acc, reinterpret_cast<float*>(smem) + wave * (32 * 36), s_tab, m0 + wm * TM * 32, n0, wn * TN * 32, lane);
            } else {
                if constexpr (WAVE_H) {
                    // fp16 tensors (a.direct == 2): a row of the 32 x 64 wave tile is one 128-B line — full-line residual loads and stores
                    if (a.direct == 2) {
                        conv_epilogue_wave_h<BN, TM>(a, acc, reinterpret_cast<float*>(smem) + wave * (32 * 68), s_tab, m0 + wm * TM * 32, n0, wn * TN * 32, lane);
                        return;
                    }
                }
                conv_epilogue_direct<T, BN, TM, TN>(a, acc, s_tab, m0 + wm * TM * 32, n0, wn * TN * 32, lane);
            }
            return;
        }
    }
    conv_epilogue<T, BN, TM, TN, WM, WN, CPASS>(a, acc, smem, m0, n0);
}

template <typename T, typename TW, int PARTS = 2>
static void conv_launch(hipStream_t s, const ConvArgs& a, int bn, bool wide_waves = false)
{
    // 8 waves as 4 (M) × 2 (N): 128×128 block tile, 32×64 per wave; narrower N tiles keep 128 rows.
    const dim3 grid(a.tiles_m * a.tiles_n * a.ksplit);
#ifndef MRCNN_RING64
#define MRCNN_RING64 3
#endif
#ifndef MRCNN_RING32
#define MRCNN_RING32 4
#endif
#ifndef MRCNN_RING128S
#define MRCNN_RING128S 3    /* split mode: a step is 8 MFMAs per wave, two tiles in flight (+2 %) */
#endif
#ifndef MRCNN_RING128H
#define MRCNN_RING128H 2    /* fp16 tensors: a third stage (96 KB) leaves one block per CU — measured, see DESIGN.md §6 */
#endif
    constexpr int R128 = (sizeof(T) == 4 && sizeof(TW) == 2) ? MRCNN_RING128S : (sizeof(T) == 2 ? MRCNN_RING128H : 2);
    if constexpr (sizeof(T) == 4 && sizeof(TW) == 2) {
        // Split modes, long K: the same 128x128 tile as 4 waves of 32x128 — one register split of an activation fragment feeds
        // four column tiles instead of two (half the split VALU and half the activation-fragment LDS reads per MFMA): +2-4 % on
        // the 3x3 layers, bit-identical (same products, same order per accumulator); short-K layers lose to its 4-wave epilogue.
        if (bn == 128 && wide_waves) { hipLaunchKernelGGL((k_conv_mfma_glds<T, TW, 128, 1, 4, 4, 1, R128, PARTS>), grid, dim3(256), 0, s, a); return; }
    }
    MRCNN_REQUIRE((a.kchunks == 1 && !a.sc_in) || (sizeof(T) == 4 && sizeof(TW) == 2 && bn != 128), MRCNN_ERR_INVALID, "conv: K chunks / a fused shortcut on a kernel that does not carry them");
    if (bn == 128) hipLaunchKernelGGL((k_conv_mfma_glds<T, TW, 128, 1, 2, 4, 2, R128, PARTS>), grid, dim3(512), 0, s, a);
    else if (bn == 64) hipLaunchKernelGGL((k_conv_mfma_glds<T, TW, 64, 1, 1, 4, 2, MRCNN_RING64, PARTS>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((k_conv_mfma_glds<T, TW, 32, 1, 1, 4, 1, MRCNN_RING32, PARTS>), grid, dim3(256), 0, s, a);
}

// The dispatcher's way in (conv_dispatch.hip).  mode: 0 fp16 tensors, 1 exact fp32, 2 / 3 split parts — conv_pp_launch's numbers
void conv_mfma_launch(hipStream_t s, const ConvArgs& a, int mode, int bn, bool wide_waves)
{
    if (mode == 0) conv_launch<_Float16, _Float16>(s, a, bn);
    else if (mode == 3) conv_launch<float, _Float16, 3>(s, a, bn, wide_waves);
    else if (mode == 2) conv_launch<float, _Float16, 2>(s, a, bn, wide_waves);
    else conv_launch<float, float>(s, a, bn);
}

}  // namespace mrcnn
