// conv_dispatch.hip — which kernel of the convolution family runs a layer (host code only: no kernel lives here).
//
// conv_forward and its fused forms (the stem, the bottleneck tail, the fp16 mode's whole bottlenecks) choose among the launches of
// kernels_conv.hip (128-row implicit GEMM), kernels_conv_pp.hip (256 x 256 ping-pong), kernels_conv_halo.hip (3x3 halo tiles, split
// modes), kernels_conv3x3_h.hip (3x3 halo tiles, fp16 mode), kernels_conv_stem.hip and kernels_bneck.hip — by the layer's shape and
// mode, the grid it makes on this chip, and the run-time switches (knobs.h).  Also here: what the launches of a thread share (the
// live profile, the fp16-range flag, the scratch owner) and the launch arguments every kernel of the family takes.
#include "conv_device.h"
#include "knobs.h"

namespace mrcnn {

void conv_mfma_launch(hipStream_t s, const ConvArgs& a, int mode, int bn, bool wide_waves);   // kernels_conv.hip: 0 fp16, 1 exact fp32, 2 / 3 split parts
void conv_pp_launch(hipStream_t s, const ConvArgs& a, int mode);   // kernels_conv_pp.hip: 0 fp16, 2 / 3 split parts
void conv_chain_launch(hipStream_t s, const ConvArgs& p, const ConvArgs& q, int parts, int n_cus, const void* p_stream, const void* q_stream);   // kernels_conv_chain.hip: split parts 2 / 3

// ---- what a layer description says about its mode and geometry --------------------------------------------------------------
static inline int conv_wdtype(const ConvDesc& d) { return d.wdtype < 0 ? d.dtype : d.wdtype; }
// fp32 activations, fp16 filters: two-pass (wdtype F16) or exact three-pass (wdtype F32X3, a filter-side tag) fp16 MFMA
static inline bool conv_is_split(const ConvDesc& d) { return d.dtype == MRCNN_F32 && (conv_wdtype(d) == MRCNN_F16 || conv_wdtype(d) == MRCNN_F32X3); }
static inline int conv_split_parts(const ConvDesc& d) { return conv_wdtype(d) == MRCNN_F32X3 ? 3 : 2; }
// fp16 tensors, fp16 filters, fp16 out
static inline bool conv_is_f16(const ConvDesc& d) { return d.dtype == MRCNN_F16 && (d.wdtype < 0 || d.wdtype == MRCNN_F16) && !d.out_f32; }
static inline bool is_pointwise(const ConvDesc& d) { return d.KH == 1 && d.KW == 1 && d.stride == 1 && !d.padH && !d.padW; }
static inline bool is_3x3_same(const ConvDesc& d) { return d.KH == 3 && d.KW == 3 && d.stride == 1 && d.padH == 1 && d.padW == 1; }
// a dense NHWC tensor of h x w pixels of c channels as the layer's input / output
static inline bool dense_in(const ConvDesc& d, int h, int w, int c) { return d.H == h && d.W == w && d.Cin == c && d.in_sW == c && d.in_sH == (long)w * c && d.in_sB == (long)h * w * c; }
static inline bool dense_out(const ConvDesc& d, int h, int w, int c) { return d.OH == h && d.OW == w && d.Cout == c && d.out_sP == c && d.out_sB == (long)h * w * c; }
// scale, shift and `act`, nothing else in the epilogue but (where the caller allows it) a plain residual
static inline bool plain_epilogue(const ConvDesc& d, int act) { return !d.out2 && !d.deconv2 && !d.sel_partial && !d.head_w && d.res_shift == 0 && d.act == act && d.scale && d.shift; }
// does a grid of one tile per block fill the chip?  (7/8 of its CUs)
static inline bool fills_chip(long tiles, int n_cus) { return tiles * 8 >= (long)n_cus * 7; }

static thread_local ConvProfile* g_prof = nullptr;
void conv_set_profiler(ConvProfile* p) { g_prof = p; }
static thread_local int* g_range_flag = nullptr;
void conv_set_range_flag(int* device_flag) { g_range_flag = device_flag; }
void ConvProfile::reset()
{
    for (auto& s : by_tile) s = Slot();
    for (auto& s : by_group) s = Slot();
    by_shape.clear();
    pending.clear();
    used = 0;
}
void ConvProfile::collect()
{
    for (auto& pd : pending) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, pool[pd.e0], pool[pd.e1]));
        by_tile[pd.tile].launches += 1;
        by_tile[pd.tile].ms += ms;
        by_tile[pd.tile].flops += pd.flops;
        by_tile[pd.tile].bytes += pd.bytes;
        Slot& sh = by_shape[pd.shape];
        sh.launches += 1; sh.ms += ms; sh.flops += pd.flops; sh.bytes += pd.bytes;
        Slot& gr = by_group[pd.group == 1 ? 1 : 0];
        gr.launches += 1; gr.ms += ms; gr.flops += pd.flops; gr.bytes += pd.bytes;
    }
    pending.clear();
    used = 0;
}
ConvProfile::~ConvProfile()
{
    for (auto e : pool) (void)hipEventDestroy(e);
}
// ALGORITHMIC bytes of a layer: every operand crosses HBM once — the input pixels the layer reads (a strided 1x1 layer: the sampled ones),
// the filters, the residual / the fused shortcut's input, the outputs it stores (fused heads: their fp32 columns instead of the feature
// tensor; selected-class mode: nothing).  What a memory-bound layer is priced against (bench.py: roofline.by_tile_class[*].frac_of_hbm).
static double conv_algorithmic_bytes(const ConvDesc& d, const ConvDesc* sc = nullptr)
{
    const double es = d.dtype == MRCNN_F16 ? 2.0 : 4.0;
    const double ws = conv_wdtype(d) == MRCNN_F32 ? 4.0 : 2.0;
    const double M = (double)d.B * d.OH * d.OW;
    const double ncols = d.deconv2 ? 4.0 * d.Cout : d.Cout;
    double b = 0;
    if (d.algo_k > 0) b += (double)d.B * d.H * d.W * 16.0;                               // the stem's staging tensor: 16 B per padded pixel
    else b += (d.KH * d.KW == 1 ? M : (double)d.B * d.H * d.W) * d.Cin * es;
    b += ncols * d.KH * d.KW * (d.algo_k > 0 ? (double)d.algo_k / (d.KH * d.KW) : (double)d.Cin) * ws;
    if (d.res) b += M * d.Cout * es / (d.res_shift ? 4.0 : 1.0);
    if (sc) b += M * sc->Cin * es + (double)d.Cout * sc->Cin * ws;
    if (d.head_w) b += M * d.head_cols * 4.0;
    else if (!d.sel_partial) b += M * ncols * (d.out_f32 ? 4.0 : es);
    return b;
}
static int prof_event(ConvProfile* p, hipStream_t s)
{
    if (p->used == (int)p->pool.size()) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        p->pool.push_back(e);
    }
    HIP_CHECK(hipEventRecord(p->pool[p->used], s));
    return p->used++;
}
// The bracket of one launch: an event before it when the calling thread's profiler is active, finish() records the one behind it
// and queues the pair for collect().
struct ProfScope {
    ConvProfile* const prof = (g_prof && g_prof->active) ? g_prof : nullptr;
    const hipStream_t s;
    const int e0;
    explicit ProfScope(hipStream_t s_) : s(s_), e0(prof ? prof_event(prof, s_) : 0) {}
    explicit operator bool() const { return prof != nullptr; }
    void finish(ConvTileClass tile, double flops, int M, int N, int K, int group, double bytes) const
    {
        const int e1 = prof_event(prof, s);
        prof->pending.push_back({tile, flops, e0, e1, {M, N, K, tile}, group, bytes});
    }
};

int conv_n_tile(int Cout)
{
    if (Cout > 64) return 128;
    if (Cout > 32) return 64;
    return 32;
}

// Run-time switches of the kernel choice (knobs.h; defaults = the shipped policy)
static int& g_min_blocks = knob("conv_min_blocks", nullptr, 448);   // narrow the N tile while the grid has fewer blocks than this: 7/8 of two blocks per CU (the
                                 // box head's 504 tiles of 128 columns beat 1008 of 64: +1.1 % end to end, tools/e2e_ab.py)
static int& g_min_blocks_split = knob("conv_min_blocks_split", nullptr, 256, "conv_min_blocks");      // ("conv_min_blocks" sets both) fp32 tensors (split modes): one block per CU is enough — a narrower tile re-reads the 4-byte activations once more per
                                 // column tile, and on a single image that L2 traffic is what the 1x1 layers wait for: 448 -> 256 is +1.2 .. 1.8 % on one image,
                                 // +0.1 % at batch 8 (profiles/r05_box_path_ab.txt); fp16 tensors keep 448 (-0.3 % at batch 8 with 256).  Same bits either way.
static inline int min_blocks_for(bool split_mode) { return split_mode ? g_min_blocks_split : g_min_blocks; }
static int& g_direct = knob("conv_direct", "MRCNN_DIRECT", 3);   // 0: every layer through the block-staged epilogue; 1: fp16 tensors straight from the accumulators;
                                 // 2: also fp32 tensors through wave-private LDS tiles (conv_epilogue_wave); 3: also the fp16 tensors of the
                                 // 128-column kernel (conv_epilogue_wave_h: full-line residual loads and stores; +3.6 % end to end in fp16 mode)
static int& g_stem = knob("conv_stem", "MRCNN_STEM", 1);        // conv1 + max-pool as one persistent launch (kernels_conv_stem.hip; split modes: bit-identical to the two launches); 2: fp16 tensors in round 4's four-group form (bit-identical to the two launches; 1 = the compact form: summation noise apart)
static int& g_tail_dbg = knob("conv_tail_dbg", "MRCNN_TAIL_DBG", 0);        // measurement only: ablation bits of the fused tail's 1x1 phase (1 no epilogue, 2 no K loop)
// Bottleneck tails (3x3 + 1x1) as one persistent launch when the grid fills the chip: bit-identical to the two launches, and
// measured SLOWER (C4, batch 8: 180 us against 88 + 75; ablations: 3x3 loop 91 + barriers / prologues 7 + staging and parking 21 +
// 1x1 K loop 21 + epilogue 37, strictly additive — profiles/r04_tail_ablate_f32x3.txt), so OFF by default;
// MRCNN_TAIL=1 / mrcnn_debug_set("conv_tail", 1) switch it on (tests keep it bit-identical)
static int& g_tail = knob("conv_tail", "MRCNN_TAIL", 0);
// fp16 mode: identity bottleneck blocks (branch2a + branch2b + branch2c + shortcut) as ONE persistent launch with the two mid tensors on chip
// (kernels_bneck.hip; bit-identical to the three launches).  MRCNN_BNECK=0 / mrcnn_debug_set("conv_bneck", 0): the three launches.
static int& g_bneck = knob("conv_bneck", "MRCNN_BNECK", 1);
// ... and (round 6) the consecutive identity blocks of a C = 256 stage — C4: 22 of ResNet-101's blocks — as ONE launch whose tiles wait for their
// neighbours' previous block instead of for a launch boundary (kernels_bneck.hip, STAGE form; bit-identical).  Measured EQUAL to one launch per
// block (profiles/r06_bneck_stage_ab.txt) and dependent on the whole grid being resident, so OFF by default: MRCNN_BNECK_STAGE=1 /
// mrcnn_debug_set("conv_bneck_stage", 1) switch it on.
static int& g_bneck_stage = knob("conv_bneck_stage", "MRCNN_BNECK_STAGE", 0);
// fp16 mode: 3x3 stride-1 layers with 256 | 512 output columns on the halo-tile / fragment-streaming kernel (kernels_conv3x3_h.hip; its own K order)
// 0: never; 1 (default): where the RPN's heads ride in its epilogue (the engine's P2..P4 levels) — as a plain 3x3 layer it equals the ping-pong kernel
// on the large levels and loses on under-filled grids (profiles/r05_c3h_ab.txt); 2: every eligible layer (tests, A/B); 3: as 1, heads as their own launch (A/B)
static int& g_c3h = knob("conv_c3h", "MRCNN_C3H", 1);
int conv_c3h_mode() { return g_c3h; }
bool conv_bneck_enabled() { return g_bneck != 0; }
// Canonical K chunks (round 4): the long-K 1x1 layers of the split modes — K >= 2048: C5's `branch2a`, the P5
// lateral, the box head's first inner product (K = 12 544) — sum their K steps as ((0 + P0) + P1) + ..., 4 / 8 equal chunks by the
// layer's shape alone, at EVERY batch.  A grid that fills the chip runs the chunks in one block (a second accumulator set, folded at
// the chunk boundaries); a grid that does not — single images: 32 tiles at C5, 64 in the box head — gives every chunk its own block
// and the last one to finish folds the partial sums in the same order: bit-identical, and the dependent chain of K steps is 4 - 8 x
// shorter (single image: 171 -> 85, 29 -> 18, 28 -> 15 us; batch 8 unchanged).
// MRCNN_KCHUNK=0 / "conv_kchunk" 0: one running sum as in rounds 1-3 (other bits); "conv_ksplit" 0: never share a tile (same bits).
// Fused shortcut (round 4, late): the first block of a ResNet stage convolves the block's input twice — `branch1` (1x1, the shortcut) and,
// three layers later, `branch2c` adds that tensor as its residual.  conv_forward(s, branch2c, &branch1) computes both in ONE launch: the
// shortcut's K loop first (its sums wait in the second accumulator set), then branch2c's, and the epilogue forms the residual from the waiting
// sums with the shortcut's own scale / shift — the same fp32 operations, bit for bit (tests/test_gpu_engine.py), and the 4 x-wide shortcut
// tensor is neither written nor read back (C2: 537 MB each way at batch 8).  "conv_scfuse" 0 / MRCNN_SCFUSE=0: the two launches.
static int& g_scfuse = knob("conv_scfuse", "MRCNN_SCFUSE", 1);
static int& g_sel_wave = knob("mask_sel_wave", "MRCNN_SEL_WAVE", 1);         // selected-class mode of the mask head's deconvolution: 1 wave-private epilogue (64-column partial sums), 0 block-staged (128)
int conv_sel_part_cols() { return g_sel_wave ? 64 : 128; }
static int& g_kchunk = knob("conv_kchunk", "MRCNN_KCHUNK", 1);
static int& g_ksplit = knob("conv_ksplit", "MRCNN_KSPLIT", 1);
static int& g_ksplit_below = knob("conv_ksplit_below", "MRCNN_KSPLIT_BELOW", 256);       // share tiles when the widest-tile grid has fewer blocks than this
static int& g_halo = knob("conv_halo", "MRCNN_HALO", 1);        // 3x3 stride-1 layers of the split modes on the halo kernel (kernels_conv_halo.hip) when the filters come re-tiled
bool conv_halo_enabled() { return g_halo != 0; }
// Split modes: a bottleneck's branch2c and the NEXT block's branch2a as one launch (kernels_conv_chain.hip; bit-identical to the two launches):
// 0 never, 1 by policy (conv_forward_chain), 2 at every grid size (tests), 3 as 2 with the entry block's shortcut riding at every grid size too (mrcnn_conv_chain_nhwc)
static int& g_chain = knob("conv_chain", "MRCNN_CHAIN", 1);
// ... and the same for C = 256 (C4's identity pairs: the ring form of kernels_conv_chain.hip): 0 never, 1 by policy, 2 at every grid size
static int& g_chain4 = knob("conv_chain4", "MRCNN_CHAIN4", 1);
static int& g_tn4 = knob("conv_tn4", nullptr, -1);       // split modes, 128x128 tile as 4 waves of 32x128: -1 by policy (conv_forward), 0 never, 1 always (tests)

// The 256 x 256 ping-pong kernel's policy.
// Shipped policy = where the A/B of tools/conv_ab.py shows a gain (profiles/r02_conv_ab_*.txt): fp16 tensors, at least two
// full rounds of 256 tiles, K >= 1024 (at K = 512 the in-engine shape table shows a loss: 564 vs 618 TFLOP/s).  The split modes run the same kernel bit-identically but no faster (both kernels
// sit at the same power-limited MFMA rate): off unless asked for.
static int& g_pp = knob("conv_pp", "MRCNN_PP", 1);
static int& g_pp_min_tiles = knob("conv_pp_min_tiles", "MRCNN_PP_MIN_TILES", 512);
static int& g_pp_min_kt = knob("conv_pp_min_kt", "MRCNN_PP_MIN_KT", 16);
static int& g_pp_dbg = knob("conv_pp_dbg", "MRCNN_PP_DBG", 0);          // ablation bits (ConvArgs::dbg)
static int& g_pp_min_fill = knob("conv_pp_min_fill", "MRCNN_PP_MIN_FILL", 85);          // percent
static int& g_pp_split = knob("conv_pp_split", "MRCNN_PP_SPLIT", 0);

// The launch arguments every kernel of the family shares (geometry, strides, epilogue fields) from a layer description.
static void conv_fill_args(const ConvDesc& d, ConvArgs& a)
{
    const bool half = d.dtype == MRCNN_F16;
    a.in = d.in; a.wgt = d.wgt; a.scale = d.scale; a.shift = d.shift; a.res = d.res; a.out = d.out; a.out2 = d.out2;
    a.in_sB = d.in_sB; a.in_sH = d.in_sH; a.in_sW = d.in_sW;
    a.res_sB = d.res_sB; a.res_sH = d.res_sH; a.res_sW = d.res_sW;
    a.out_sB = d.out_sB; a.out_sP = d.out_sP; a.out_sH = d.out_sH; a.out_sW = d.out_sW;
    a.out2_sB = d.out2_sB; a.out2_sP = d.out2_sP;
    a.B = d.B; a.H = d.H; a.W = d.W; a.Cin = d.Cin; a.KH = d.KH; a.KW = d.KW; a.stride = d.stride; a.padH = d.padH; a.padW = d.padW;
    a.OH = d.OH; a.OW = d.OW; a.Cout = d.Cout;
    a.ncols = d.deconv2 ? 4 * d.Cout : d.Cout;
    a.Ktot = d.KH * d.KW * d.Cin;
    const long M = (long)d.B * d.OH * d.OW;
    MRCNN_REQUIRE(M > 0 && M < (1L << 31) - 256, MRCNN_ERR_SHAPE, "conv: M out of range");
    a.M = (int)M;
    a.res_shift = d.res_shift; a.act = d.act; a.n_split = d.n_split; a.deconv2 = d.deconv2;
    a.out_f32 = (!half || d.out_f32) ? 1 : 0;
    a.range_flag = g_range_flag;
    a.dbg = g_pp_dbg;
    a.sel_w = d.sel_w; a.sel_cid = d.sel_cid; a.sel_partial = d.sel_partial;
    a.kchunks = 1; a.ksplit = 1; a.ks_scratch = nullptr; a.ks_count = nullptr;
    a.sel_part_cols = 128;
    a.sc_in = nullptr; a.sc_wgt = nullptr; a.sc_scale = nullptr; a.sc_shift = nullptr;
    a.sc_in_sB = a.sc_in_sH = a.sc_in_sW = 0; a.sc_H = a.sc_W = a.sc_Cin = 0; a.sc_stride = 1;
}

// Canonical K chunks of a layer (1 = one running sum): by its shape and mode alone — never by the batch or the grid
int conv_k_chunks(const ConvDesc& d)
{
    // (K = 1024 — C4's branch2a, the box head's second inner product — is left as one sum: two chunks gain 1.2 us per launch on a
    //  single image and cost 1.5 us at batch 8 for the second accumulator set, gpurun_out/r4w)
    if (!g_kchunk || !conv_is_split(d) || d.KH != 1 || d.KW != 1 || d.Cin < 2048 || d.Cin % 32 != 0 || d.head_w) return 1;
    int n = d.Cin >= 8192 ? 8 : 4;
    while ((d.Cin / 32) % n) n >>= 1;
    return n;
}

// Partial sums of shared tiles: 64 MB + 8192 counters per stream, allocated at the stream's first shared launch and kept (a
// captured graph holds the pointers; the engine's first predict at a batch size runs eagerly, so the allocation never falls
// inside a capture).  Launches on one stream are ordered, and a launch leaves its counters at zero.
static constexpr size_t KS_BYTES = 64u << 20;
static constexpr int KS_TILES = 8192;
static thread_local ConvScratch* g_scratch = nullptr;
void conv_set_scratch(ConvScratch* c) { g_scratch = c; }
size_t ConvScratch::ks_bytes() { return KS_BYTES; }
void ConvScratch::alloc()
{
    ks_buf.alloc(KS_BYTES);
    ks_cnt.alloc(KS_TILES * sizeof(unsigned));
    HIP_CHECK(hipMemset(ks_cnt.p, 0, KS_TILES * sizeof(unsigned)));       // (every launch leaves the counters at zero)
}
ConvScratch* conv_current_scratch() { return g_scratch; }

// May the epilogue use 16-B vector stores / residual loads for this layer?
static int conv_vec_ok(const ConvDesc& d, const ConvArgs& a)
{
    const bool half = d.dtype == MRCNN_F16;
    auto al = [](const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; };
    const int cpt = half ? 8 : 4;        // columns per epilogue thread: 16 B of the activation type
    return a.ncols % cpt == 0 && d.out2 == nullptr && d.out_sP % cpt == 0 && d.out_sB % cpt == 0 && al(d.out, 16) &&
               (!d.scale || al(d.scale, 16)) && (!d.shift || al(d.shift, 16)) &&
               (!d.res || (d.res_sW % cpt == 0 && d.res_sH % cpt == 0 && d.res_sB % cpt == 0 && al(d.res, 16))) &&
               (!d.deconv2 || (d.Cout % cpt == 0 && d.out_sH % cpt == 0 && d.out_sW % cpt == 0));
}

// May `main` (a 1x1 layer whose residual is exactly the output of the 1x1 layer `sc`) absorb `sc`?  (conv_forward checks the tile and the epilogue form.)
static bool conv_shortcut_fusable(const ConvDesc& m, const ConvDesc& sc)
{
    if (!conv_is_split(m) || !conv_is_split(sc) || conv_wdtype(m) != conv_wdtype(sc)) return false;          // split modes
    if (m.KH != 1 || m.KW != 1 || sc.KH != 1 || sc.KW != 1 || m.padH || m.padW || sc.padH || sc.padW || m.stride != 1) return false;
    if (m.B != sc.B || m.OH != sc.OH || m.OW != sc.OW || m.Cout != sc.Cout || m.Npad != sc.Npad || sc.Cin % 32 != 0) return false;
    if (sc.act != ACT_NONE || sc.res || sc.out2 || sc.deconv2 || sc.sel_partial || sc.head_w || m.out2 || m.deconv2 || m.sel_partial || m.head_w || m.act == ACT_SIGMOID) return false;
    // the residual IS the shortcut's output, element for element
    if (m.res != sc.out || m.res_shift != 0 || m.res_sW != sc.out_sP || m.res_sB != sc.out_sB || m.res_sH != (long)m.OW * m.res_sW) return false;
    if (sc.out_sB != (long)sc.OH * sc.OW * sc.out_sP) return false;
    return true;
}

// Does `sc` ride in d_in's launch (conv_forward), or run first as its own?
static bool conv_shortcut_rides(const ConvDesc& d_in, const ConvDesc* sc)
{
    bool fuse = sc && g_scfuse && conv_shortcut_fusable(d_in, *sc) && conv_k_chunks(d_in) == 1 && conv_k_chunks(*sc) == 1;
    if (fuse) {
        // the fused form needs the direct fp32 epilogue (tiles of 64 columns or more)
        const int bn_max = conv_n_tile(d_in.Cout);
        int bn = bn_max;
        const long tiles_m = ((long)d_in.B * d_in.OH * d_in.OW + BM_DEFAULT - 1) / BM_DEFAULT;
        while (bn > 32 && tiles_m * (d_in.Npad / bn) < min_blocks_for(true)) bn >>= 1;          // (fused shortcuts exist in the split modes only)
        ConvDesc probe = d_in;
        probe.res = nullptr;
        ConvArgs pa;
        conv_fill_args(probe, pa);
        if (bn < 64 || g_direct < 2 || !conv_vec_ok(probe, pa)) fuse = false;
#ifndef MRCNN_CONV_ABLATE
        if (g_pp_dbg) fuse = false;          // (the measurement build ablates the fused launch too)
#endif
    }
    return fuse;
}

void conv_forward(hipStream_t s, const ConvDesc& d_in, const ConvDesc* sc)
{
    // a shortcut that cannot ride in this launch runs first, as its own (its output is this layer's residual)
    const bool fuse = conv_shortcut_rides(d_in, sc);
    if (sc && !fuse) conv_forward(s, *sc, nullptr);
    ConvDesc d = d_in;
    if (fuse) { d.res = nullptr; d.res_sB = d.res_sH = d.res_sW = 0; }
    const bool half = d.dtype == MRCNN_F16;
    const int wdtype = conv_wdtype(d);
    if (half && g_c3h && (d.head_w || d.prefer_c3h || g_c3h == 2) && conv3x3h_eligible(d)) {
        const int n_cus_c3h = device_cu_count();
        const ProfScope prof(s);
        conv3x3h_launch(s, d, g_range_flag, n_cus_c3h);
        if (prof) {
            const double M = (double)d.B * d.OH * d.OW;
            prof.finish(TILE_C3H, 2.0 * M * d.Cout * 9.0 * d.Cin, (int)M, d.Cout, 9 * d.Cin, d.group, conv_algorithmic_bytes(d));
        }
        return;
    }
    const bool split = conv_is_split(d);
    const int parts = conv_split_parts(d);
    MRCNN_REQUIRE(d.dtype == MRCNN_F32 || half, MRCNN_ERR_UNSUPPORTED, "conv: dtype %d", d.dtype);
    MRCNN_REQUIRE(wdtype == d.dtype || split, MRCNN_ERR_UNSUPPORTED, "conv: activation dtype %d with filter dtype %d", d.dtype, wdtype);
    const int bk = half ? 64 : 32;
    MRCNN_REQUIRE(d.Cin % bk == 0, MRCNN_ERR_SHAPE, "conv: Cin %d not a multiple of %d", d.Cin, bk);
    ConvArgs a;
    conv_fill_args(d, a);
    MRCNN_REQUIRE(!d.sel_partial || (d.deconv2 && d.sel_w && d.sel_cid && d.Cout % 128 == 0 && d.Npad == 4 * d.Cout && !d.out2),
                  MRCNN_ERR_INVALID, "conv: the selected-class mode needs a 2x2 transposed convolution with Cout a multiple of 128");
    // Tile choice: the widest N tile the packed weights allow, narrowed while the grid would leave
    // the chip under-filled (< 7/8 of 2 blocks per CU) — C5, the top FPN levels and the small RPN levels.
    const int bn_max = conv_n_tile(a.ncols);
    MRCNN_REQUIRE(d.Npad % bn_max == 0 && d.Npad >= a.ncols, MRCNN_ERR_SHAPE, "conv: Npad %d incompatible with tile %d", d.Npad, bn_max);
    a.tiles_m = (a.M + BM_DEFAULT - 1) / BM_DEFAULT;
    int bn = bn_max;
    while (bn > 32 && !d.sel_partial && (long)a.tiles_m * (d.Npad / bn) < min_blocks_for(split)) bn >>= 1;     // (selected-class mode: fixed 128-channel parts)
    if (fuse) {
        a.sc_in = sc->in; a.sc_wgt = sc->wgt; a.sc_scale = sc->scale; a.sc_shift = sc->shift;
        a.sc_in_sB = sc->in_sB; a.sc_in_sH = sc->in_sH; a.sc_in_sW = sc->in_sW;
        a.sc_H = sc->H; a.sc_W = sc->W; a.sc_Cin = sc->Cin; a.sc_stride = sc->stride;
    }
    // (a fused shortcut needs the second accumulator set: the eight-wave 128-column form has no registers for it; of the two forms that do,
    //  the four-wave 128-column one measured C2 / C3 / C4 / C5 321 / 247 / 171 / 150 us against 355 / 282 / 221 / 193 for the eight-wave
    //  64-column one, and 430 / 288 / 180 / 159 for the two launches each replaces: gpurun_out/r5g)
    a.kchunks = d.sel_partial ? 1 : conv_k_chunks(d);
    if (a.kchunks > 1 && g_ksplit && (long)a.tiles_m * (d.Npad / bn_max) < g_ksplit_below) {
        // an under-filled grid: one block per (tile, chunk), the N tile as wide as the shared grid allows
        int bs = bn_max;
        while (bs > 32 && (long)a.tiles_m * (d.Npad / bs) * a.kchunks < min_blocks_for(true)) bs >>= 1;
        const long tiles = (long)a.tiles_m * (d.Npad / bs);
        // (the shared-tile form needs the owner's scratch: a launch without one keeps its chunks in one block — the same bits)
        if (g_scratch && g_scratch->ks_buf.p && tiles <= KS_TILES && (size_t)tiles * a.kchunks * BM_DEFAULT * bs * 4 <= KS_BYTES) {
            bn = bs;
            a.ksplit = a.kchunks;
            a.ks_scratch = g_scratch->ks_buf.as<float>();
            a.ks_count = g_scratch->ks_cnt.as<unsigned>();
        }
    }
    a.vec_ok = conv_vec_ok(d, a);
    a.tiles_n = d.Npad / bn;
    MRCNN_REQUIRE(!d.sel_partial || (bn == 128 && a.vec_ok), MRCNN_ERR_INVALID, "conv: the selected-class mode needs the 128-wide vector epilogue");
    // Epilogue without block barriers wherever the layer allows: fp32 tensors through wave-private LDS tiles (conv_epilogue_wave:
    // full-line stores — a lane's own 16-B store would hold four channels of one pixel, 64 scattered pieces per instruction, which
    // lost 1.4 % — without the two barriers of the block-staged form: +1.6 % end to end, tools/e2e_direct_ab.sh, round 3); fp16
    // tensors of the 128-column kernel the same way (conv_epilogue_wave_h: a row of the 32 x 64 wave tile is one 128-B line;
    // +3.6 % end to end in fp16 mode over the form below, tools/e2e_ab.py f16 conv_direct 2 3), the narrower fp16 tiles straight
    // from the accumulators (conv_epilogue_direct: 32-B pieces per pixel and store, +0.9 % over the block-staged form).
    a.direct = (g_direct && (half || g_direct > 1) && a.vec_ok && !d.out2 && !d.deconv2 && d.act != ACT_SIGMOID && (!half || !a.out_f32)) ? 1 : 0;
    MRCNN_REQUIRE(!fuse || (a.direct && bn >= 64), MRCNN_ERR_INVALID, "conv: fused shortcut without the direct epilogue (conv_forward's own check should have said so)");
    if (a.direct && half && g_direct > 2) a.direct = 2;      // fp16 tensors through wave-private tiles where the wave tile is 32 x 64 (the 128-column kernel)
    // selected-class mode: the wave-private form (64-column partial sums straight from the accumulators) on the eight-wave 128-column kernel
    if (d.sel_partial && g_sel_wave && bn == 128 && a.vec_ok && d.act != ACT_SIGMOID && d.Cout % 64 == 0) { a.direct = 1; a.sel_part_cols = 64; }
    // Layers with a large GEMM: the 256×256 persistent ping-pong kernel (kernels_conv_pp.hip), one block per CU — when the
    // tiles fill whole rounds of the chip well enough (a static walk: the last round costs as much as a full one).
    int pp_bn = 0;
    {
        const long tiles = (long)((a.M + 255) / 256) * (d.Npad / 256);
        const long rounds = (tiles + 255) / 256;
        const bool fills = tiles >= g_pp_min_tiles && tiles * 100 >= rounds * 256 * g_pp_min_fill;
        const int bk_pp = half ? 64 : 32;
        if (g_pp && (half || (split && g_pp_split)) && d.Cin % bk_pp == 0 && a.Ktot / bk_pp >= g_pp_min_kt && d.Npad % 256 == 0 && fills &&
            a.kchunks == 1 && !fuse && a.vec_ok && (!half || !a.out_f32) && !d.deconv2 && !d.out2 && d.act != ACT_SIGMOID && d.H < 32760 && d.W < 32760)
            pp_bn = 256;                    // ... and the epilogue / address forms pp_store_tile and PP_SRC_A cover
    }
    if (pp_bn) { a.tiles_m = (a.M + 255) / 256; a.tiles_n = d.Npad / pp_bn; }
    // K >= 2048: the 3x3 layers; and every chunked layer (the 8-wave form has no registers for the second accumulator set)
    // (selected-class mode: its wave-private epilogue exists for the eight-wave tile only, and the partial-sum layout the caller sized
    //  — conv_sel_part_cols — must not depend on K or on "conv_tn4": the four-wave form would return without a single store)
    const bool wide_waves = split && bn == 128 && !d.sel_partial && (a.kchunks > 1 || fuse || (g_tn4 < 0 ? a.Ktot / bk >= 64 : g_tn4 != 0));
    const ProfScope prof(s);
    // 3x3 stride-1 layers of the split modes: the persistent halo kernel, whenever the layer qualifies — by its geometry and
    // mode alone, so that a layer runs in ONE summation order whatever the batch (the kernel's K order is its own).
    const bool halo = g_halo && d.wgt_halo && a.vec_ok && conv_halo_eligible(d);
    MRCNN_REQUIRE(!d.head_w || (halo && conv_halo_head_eligible(d)), MRCNN_ERR_INVALID, "conv: a fused head needs the halo kernel (layer not eligible, or switched off)");
    if (halo) {
        const int n_cus = device_cu_count();
        pp_bn = 0;
        (void)conv_halo_forward(s, a, d, parts, n_cus);
    } else
    if (pp_bn) conv_pp_launch(s, a, half ? 0 : parts);
    else conv_mfma_launch(s, a, half ? 0 : (split ? parts : 1), bn, wide_waves);
    if (prof) {
        const double k = (d.algo_k > 0 ? d.algo_k : a.Ktot) + (fuse ? sc->Cin : 0);          // (a fused shortcut: both K loops)
        const ConvTileClass tile = halo ? TILE_HALO : pp_bn == 256 ? TILE_PP_256x256 : (wide_waves ? TILE_128x128_4WAVE : (bn == 128 ? TILE_128x128 : (bn == 64 ? TILE_128x64 : TILE_128x32)));
        prof.finish(tile, 2.0 * (double)a.M * (double)a.ncols * k, a.M, a.ncols, a.Ktot, d.group, conv_algorithmic_bytes(d, fuse ? sc : nullptr));
    }
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Fused stem (kernels.h: conv_stem_forward)
// ------------------------------------------------------------------------------------------------
bool conv_stem_enabled() { return g_stem != 0; }
bool conv_stem_eligible(const ConvDesc& d)
{
    const bool half = conv_is_f16(d);
    const int pxc = half ? 8 : 4;          // channels of a staged pixel: 16 B either way
    return (conv_is_split(d) || half) && d.KH == 7 && d.KW == 1 && d.Cin == 8 * pxc && d.stride == 2 && d.padH == 0 && d.padW == 0 && d.Cout == 64 && d.Npad == 64 &&
           d.act == ACT_RELU && !d.res && !d.out2 && !d.deconv2 && d.in_sW == pxc && d.in_sH == (long)d.W * pxc && d.in_sB == (long)d.H * d.W * pxc &&
           d.OH == (d.H - 7) / 2 + 1 && d.OW == (d.W - 7) / 2 + 1;
}

void conv_stem_forward(hipStream_t s, const ConvDesc& d, void* pooled, int PH, int PW)
{
    MRCNN_REQUIRE(conv_stem_eligible(d) && pooled && PH == (d.OH + 1) / 2 && PW == (d.OW + 1) / 2, MRCNN_ERR_INVALID, "conv_stem_forward: not the stem layer");
    const int n_cus = device_cu_count();
    const ProfScope prof(s);
    conv_stem_launch(s, d.in, d.B, d.H, d.W, d.wgt, d.scale, d.shift, d.OH, d.OW, pooled, PH, PW,
                     d.dtype == MRCNN_F16 ? 1 : conv_split_parts(d), g_range_flag, n_cus, g_stem != 2);
    if (prof) {
        const long M = (long)d.B * d.OH * d.OW;
        const double k = d.algo_k > 0 ? d.algo_k : d.KH * d.KW * d.Cin;
        // (the 64-column class of the table: the layer it replaces ran there; the pool rides in the same launch)
        // algorithmic bytes: the staging tensor in, the POOLED tensor out (conv1's own output never exists)
        const double by = (double)d.B * d.H * d.W * 16.0 + 64.0 * k * 2.0 + (double)d.B * PH * PW * 64.0 * (d.dtype == MRCNN_F16 ? 2.0 : 4.0);
        prof.finish(TILE_128x64, 2.0 * (double)M * 64.0 * k, (int)M, 64, d.KH * d.KW * d.Cin, d.group, by);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused bottleneck tail (kernels.h: conv_forward_tail)
// ------------------------------------------------------------------------------------------------
bool conv_tail_fusable(const ConvDesc& d3, const ConvDesc& d1)
{
    if (!conv_is_split(d3) || !conv_is_split(d1) || conv_wdtype(d3) != conv_wdtype(d1)) return false;      // split modes only
    if (!d3.wgt_halo || !d1.wgt_halo || !conv_halo_eligible(d3) || d3.head_w || !conv_halo_tail_geometry_ok(d3.H, d3.W)) return false;
    if (d3.Npad != 256 || d3.act != ACT_RELU) return false;
    if (!conv_halo_tail_packable(d1.KH, d1.KW, d1.Cin, d1.Npad) || d1.Cout != 1024 || !is_pointwise(d1)) return false;
    if (d1.deconv2 || d1.out2 || d1.sel_partial || d1.act == ACT_SIGMOID || d1.res_shift || d1.head_w) return false;
    // the 1x1 reads exactly what the 3x3 writes: a dense NHWC tensor of 256 channels
    if (d1.in != d3.out || d1.B != d3.B || d1.OH != d3.OH || d1.OW != d3.OW) return false;
    if (!dense_out(d3, d3.OH, d3.OW, 256) || !dense_in(d1, d3.OH, d3.OW, 256)) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------
// Chained pair (kernels.h: conv_forward_chain)
// ------------------------------------------------------------------------------------------------
bool conv_chain_fusable(const ConvDesc& dP, const ConvDesc& dQ, const ConvDesc* sc)
{
    if (!conv_is_split(dP) || !conv_is_split(dQ) || conv_wdtype(dP) != conv_wdtype(dQ)) return false;      // split modes, one filter dtype
    const int C = dQ.Cout, H = dP.OH, W = dP.OW;
    if (!(C == 64 || C == 128 || C == 256) || dQ.Npad != C || dP.Cin != C || dP.Cout != 4 * C || dP.Npad != 4 * C) return false;
    if (!is_pointwise(dP) || !is_pointwise(dQ) || dP.B != dQ.B) return false;
    if (!plain_epilogue(dP, ACT_RELU) || !plain_epilogue(dQ, ACT_RELU) || dQ.res) return false;
    if (!dense_in(dP, H, W, C) || !dense_out(dP, H, W, 4 * C) || dQ.in != dP.out || !dense_in(dQ, H, W, 4 * C) || !dense_out(dQ, H, W, C)) return false;
    if (conv_k_chunks(dP) != 1 || conv_k_chunks(dQ) != 1) return false;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(dP.in) || !al(dP.out) || !al(dQ.out) || !al(dP.wgt) || !al(dQ.wgt) || !al(dP.scale) || !al(dP.shift) || !al(dQ.scale) || !al(dQ.shift)) return false;
    // C = 256 (the ring form): identity pairs only, both filters as stream images
    if (C == 256 && (sc || !dP.wgt_stream || !dQ.wgt_stream || !al(dP.wgt_stream) || !al(dQ.wgt_stream))) return false;
    if (sc) {
        // the residual is formed from the shortcut's sums, as conv_forward does it
        if (!g_scfuse || !conv_shortcut_fusable(dP, *sc) || conv_k_chunks(*sc) != 1 || !sc->scale || !sc->shift) return false;
        if (C == 64 && sc->Cin != 64) return false;          // (C = 64 runs with every filter resident in LDS: the shortcut's too)
        if (!al(sc->in) || !al(sc->wgt) || !al(sc->scale) || !al(sc->shift) || sc->in_sW % 4 || sc->in_sH % 4 || sc->in_sB % 4 || sc->Npad != 4 * C) return false;
    } else {
        if (!dP.res || !al(dP.res) || dP.res_sW != 4 * C || dP.res_sH != (long)W * 4 * C || dP.res_sB != (long)H * W * 4 * C) return false;
    }
    return true;
}

void conv_forward_chain(hipStream_t s, const ConvDesc& dP, const ConvDesc& dQ, const ConvDesc* sc)
{
    const long tiles = ((long)dP.B * dP.OH * dP.OW + 127) / 128;
    // a shortcut rides in the chained launch exactly where it would ride in dP's own (conv_forward): the chain removes dQ's launch and no other
    // ("conv_chain" 3, the test entry: the shortcut rides wherever the pair qualifies — the small shapes of tests/test_gpu_conv_chain.py reach that form)
    const bool sc_rides = g_chain >= 3 ? sc != nullptr && conv_chain_fusable(dP, dQ, sc) : conv_shortcut_rides(dP, sc);
    // By policy ("conv_chain" 1) a pair is chained where the grid fills the chip AND its shape pays: C = 64 (C2), whose filters stay resident in LDS.
    // C = 128 (C3) — 256 KB of filters, fetched from L2 by every wave — measured SLOWER than its two launches: excluded by shape.
    // C = 256 (C4) — 1 MB of filters, streamed through a block-shared LDS ring — has its own knob; a dP that carries the stage's shortcut (fused, or
    // as the tensor it adds) is never chained there.
    const int n_cus = device_cu_count();
    const bool c4 = dQ.Cout == 256;
    const int g = c4 ? g_chain4 : g_chain;
    bool chain = g && g_direct >= 2 && !(c4 && sc) && conv_chain_fusable(dP, dQ, sc_rides ? sc : nullptr) && (g >= 2 || ((c4 || dQ.Cout == 64) && fills_chip(tiles, n_cus)));
#ifndef MRCNN_CONV_ABLATE
    if (g_pp_dbg) chain = false;
#endif
    if (!chain) {
        conv_forward(s, dP, sc);
        conv_forward(s, dQ);
        return;
    }
    if (sc && !sc_rides) { conv_forward(s, *sc); sc = nullptr; }          // (its output is dP's residual)
    ConvDesc d = dP;
    if (sc) { d.res = nullptr; d.res_sB = d.res_sH = d.res_sW = 0; }
    ConvArgs aP, aQ;
    conv_fill_args(d, aP);
    conv_fill_args(dQ, aQ);
    if (sc) {
        aP.sc_in = sc->in; aP.sc_wgt = sc->wgt; aP.sc_scale = sc->scale; aP.sc_shift = sc->shift;
        aP.sc_in_sB = sc->in_sB; aP.sc_in_sH = sc->in_sH; aP.sc_in_sW = sc->in_sW;
        aP.sc_H = sc->H; aP.sc_W = sc->W; aP.sc_Cin = sc->Cin; aP.sc_stride = sc->stride;
    }
    const ProfScope prof(s);
    conv_chain_launch(s, aP, aQ, conv_split_parts(dP), n_cus, dP.wgt_stream, dQ.wgt_stream);
    if (prof) {
        // one launch, two layers, under the tile class P's own launch has: the flops of both, the bytes of both less Q's input read
        const double fl = 2.0 * (double)aP.M * ((double)aP.ncols * (aP.Ktot + (sc ? sc->Cin : 0)) + (double)aQ.ncols * aQ.Ktot);
        prof.finish(sc ? TILE_128x128_4WAVE : TILE_128x128, fl, aP.M, aP.ncols, aP.Ktot, dP.group,
                    conv_algorithmic_bytes(d, sc) + conv_algorithmic_bytes(dQ) - (double)aP.M * dQ.Cin * 4.0);
    }
    HIP_CHECK(hipGetLastError());
}

void conv_forward_tail(hipStream_t s, const ConvDesc& d3, const ConvDesc& d1, const ConvDesc* sc, const ConvDesc* q)
{
    const int n_cus = device_cu_count();
    const long tiles = ((long)d3.B * d3.OH * d3.OW + 127) / 128;
    ConvArgs a3, a1;
    bool fuse = g_tail && g_halo && g_scratch && conv_tail_fusable(d3, d1) && fills_chip(tiles, n_cus);       // a grid that fills the chip: one 128 x 256 tile per block (and an owner for the parking buffer)
    if (sc && fuse) { conv_forward(s, *sc); sc = nullptr; }          // (the fused tail reads its residual from memory: the shortcut runs as its own launch)
    if (fuse) {
        conv_fill_args(d3, a3);
        conv_fill_args(d1, a1);
        a3.vec_ok = conv_vec_ok(d3, a3);
        a1.vec_ok = conv_vec_ok(d1, a1);
        a3.tiles_m = a1.tiles_m = 0; a3.tiles_n = a1.tiles_n = 0; a3.direct = a1.direct = 1;
        a1.dbg = g_tail_dbg;
        fuse = a3.vec_ok && a1.vec_ok && a3.dbg == 0;
    }
    if (!fuse) {
        conv_forward(s, d3);
        if (q) conv_forward_chain(s, d1, *q, sc);
        else conv_forward(s, d1, sc);
        return;
    }
    const ProfScope prof(s);
    (void)conv_halo_forward(s, a3, d3, conv_split_parts(d3), n_cus, &a1, d1.wgt_halo);
    if (prof) {
        // one launch, two layers: algorithmic flops of both; the shape key is the 3x3 layer's M and K with the 1x1's N (tile class 6)
        const double fl = 2.0 * (double)a3.M * ((double)a3.ncols * a3.Ktot + (double)a1.ncols * a1.Ktot);
        ConvDesc d3n = d3; d3n.sel_partial = (float*)1;          // (the tensor between the two layers is not stored: count d3 without its output)
        prof.finish(TILE_HALO_TAIL, fl, a3.M, a1.ncols, a3.Ktot + a1.Ktot, d3.group, conv_algorithmic_bytes(d3n) + conv_algorithmic_bytes(d1) - (double)a3.M * d1.Cin * 4.0);
    }
    HIP_CHECK(hipGetLastError());
    if (q) conv_forward(s, *q);          // (the fused tail stores d1's output itself: the next layer runs as its own launch)
}

// ------------------------------------------------------------------------------------------------
// Fused identity bottleneck of the fp16 mode (kernels.h: conv_bneck_forward)
// ------------------------------------------------------------------------------------------------
bool conv_bneck_fusable(const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc)
{
    if (!conv_is_f16(da) || !conv_is_f16(db) || !conv_is_f16(dc)) return false;
    const int C = da.Cout, H = da.H, W = da.W;
    if (!(C == 64 || C == 128 || C == 256) || !bneck_geometry_ok(C, H, W)) return false;
    if (!plain_epilogue(da, ACT_RELU) || !plain_epilogue(db, ACT_RELU) || !plain_epilogue(dc, ACT_RELU) || da.res || db.res) return false;
    if (!is_pointwise(da) || !dense_in(da, H, W, 4 * C) || !dense_out(da, H, W, C)) return false;
    if (!is_3x3_same(db) || db.in != da.out || !dense_in(db, H, W, C) || !dense_out(db, H, W, C)) return false;
    if (!is_pointwise(dc) || dc.in != db.out || !dense_in(dc, H, W, C) || !dense_out(dc, H, W, 4 * C)) return false;
    if (dc.res != da.in || dc.res_sW != 4 * C || dc.res_sH != (long)W * 4 * C || dc.res_sB != (long)H * W * 4 * C) return false;
    if (dc.out == da.in) return false;                // a tile reads halo pixels its neighbours own
    if (da.B != db.B || da.B != dc.B) return false;
    return true;
}

void conv_bneck_forward(hipStream_t s, const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc)
{
    const int n_cus = device_cu_count();
    // One tile per block: a grid that leaves the chip under-filled (single images: 32 tiles at C4) runs the three launches, whose narrower
    // tiles spread over more CUs — the two forms agree bit for bit, so the choice may follow the batch (measured at batch 1, fp16 mode:
    // 2.66 ms per image with the three launches, 3.59 fused everywhere; batch 8: 9.87 -> 9.52 ms fused)
    const int C_ = da.Cout;
    const long ntiles = (long)da.B * (da.H / (C_ == 256 ? 8 : 16)) * (da.W / 16);
    if (!g_bneck || !conv_bneck_fusable(da, db, dc) || (g_bneck < 3 && !fills_chip(ntiles, n_cus))) {      // ("conv_bneck" 3: fused at every grid size, tests)
        conv_forward(s, da);
        conv_forward_tail(s, db, dc, nullptr);
        return;
    }
    const ProfScope prof(s);
    bneck_launch(s, da.Cout, da.in, dc.out, da.B, da.H, da.W, da.wgt, db.wgt, dc.wgt, da.scale, da.shift, db.scale, db.shift, dc.scale, dc.shift,
                 g_range_flag, n_cus, g_bneck >= 2 ? nullptr : db.wgt_frag, g_bneck >= 2 ? nullptr : dc.wgt_frag, g_bneck >= 2 ? nullptr : da.wgt_frag);      // ("conv_bneck" 2: every operand through LDS)
    if (prof) {
        const double M = (double)da.B * da.H * da.W, C = da.Cout;
        const double fl = 2.0 * M * (4 * C * C + 9 * C * C + 4 * C * C);      // algorithmic flops of the three layers (the halo recompute is not work)
        prof.finish(TILE_BNECK, fl, (int)M, 4 * da.Cout, 17 * da.Cout, da.group, 2.0 * M * 4 * C * 2.0 + 17.0 * C * C * 2.0);      // x in + y out + the filters
    }
}

void conv_bneck_stage_forward(hipStream_t s, const BneckTriple* blocks, int n, const void* layers_dev, unsigned* done)
{
    const int n_cus = device_cu_count();
    bool stage = n >= 2 && g_bneck == 1 && g_bneck_stage && layers_dev && done && g_range_flag;
    if (stage) {
        const ConvDesc& a0 = blocks[0].a;
        const long ntiles = (long)a0.B * (a0.H / 8) * (a0.W / 16);
        stage = a0.Cout == 256 && fills_chip(ntiles, n_cus);           // the per-block rule: an under-filled grid runs the three launches
        for (int i = 0; i < n && stage; ++i) {
            const BneckTriple& t = blocks[i];
            stage = conv_bneck_fusable(t.a, t.b, t.c) && t.a.wgt_frag && t.b.wgt_frag && t.c.wgt_frag && t.a.Cout == 256 && t.a.B == a0.B && t.a.H == a0.H && t.a.W == a0.W;
            if (i > 0) stage = stage && t.a.in == blocks[i - 1].c.out && (i < 2 || t.c.out == blocks[i - 2].c.out);      // a chain between two tensors
        }
        stage = stage && blocks[1].c.out == a0.in;
    }
    if (!stage) {
        for (int i = 0; i < n; ++i) conv_bneck_forward(s, blocks[i].a, blocks[i].b, blocks[i].c);
        return;
    }
    const ConvDesc& a0 = blocks[0].a;
    const ProfScope prof(s);
    bneck_stage_launch(s, layers_dev, n, const_cast<void*>(a0.in), blocks[0].c.out, a0.B, a0.H, a0.W, done, g_range_flag, n_cus);
    if (prof) {
        const double M = (double)a0.B * a0.H * a0.W, C = a0.Cout;
        const double fl = 2.0 * M * (4 * C * C + 9 * C * C + 4 * C * C) * n;      // algorithmic flops of the n blocks
        prof.finish(TILE_BNECK, fl, (int)M, 4 * a0.Cout, 17 * a0.Cout * n, a0.group, (2.0 * M * 4 * C * 2.0 + 17.0 * C * C * 2.0) * n);
    }
}

bool conv_bneck_first_fusable(const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc, const ConvDesc& ds)
{
    if (!conv_is_f16(da) || !conv_is_f16(db) || !conv_is_f16(dc) || !conv_is_f16(ds)) return false;
    const int C = da.Cout, H = da.H, W = da.W;
    if (C != 64 || da.Cin != C || !bneck_geometry_ok(C, H, W)) return false;
    if (!plain_epilogue(da, ACT_RELU) || !plain_epilogue(db, ACT_RELU) || !plain_epilogue(dc, ACT_RELU) || !plain_epilogue(ds, ACT_NONE) || da.res || db.res || ds.res) return false;
    if (!is_pointwise(da) || !dense_in(da, H, W, C) || !dense_out(da, H, W, C)) return false;
    if (!is_pointwise(ds) || ds.in != da.in || !dense_in(ds, H, W, C) || !dense_out(ds, H, W, 4 * C)) return false;
    if (!is_3x3_same(db) || db.in != da.out || !dense_in(db, H, W, C) || !dense_out(db, H, W, C)) return false;
    if (!is_pointwise(dc) || dc.in != db.out || !dense_in(dc, H, W, C) || !dense_out(dc, H, W, 4 * C)) return false;
    if (dc.res != ds.out || dc.res_sW != 4 * C || dc.res_sH != (long)W * 4 * C || dc.res_sB != (long)H * W * 4 * C) return false;
    if (dc.out == da.in || da.B != db.B || da.B != dc.B || da.B != ds.B) return false;
    return true;
}

void conv_bneck_first_forward(hipStream_t s, const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc, const ConvDesc& ds)
{
    const int n_cus = device_cu_count();
    const long ntiles = (long)da.B * (da.H / 16) * (da.W / 16);
    if (!g_bneck || !conv_bneck_first_fusable(da, db, dc, ds) || (g_bneck < 3 && !fills_chip(ntiles, n_cus))) {
        conv_forward(s, da);
        conv_forward_tail(s, db, dc, &ds);
        return;
    }
    const ProfScope prof(s);
    bneck_launch(s, da.Cout, da.in, dc.out, da.B, da.H, da.W, da.wgt, db.wgt, dc.wgt, da.scale, da.shift, db.scale, db.shift, dc.scale, dc.shift,
                 g_range_flag, n_cus, nullptr, nullptr, nullptr, ds.wgt, ds.scale, ds.shift);
    if (prof) {
        const double M = (double)da.B * da.H * da.W, C = da.Cout;
        const double fl = 2.0 * M * (C * C + 9 * C * C + 4 * C * C + 4 * C * C);       // branch2a, 2b, 2c and branch1
        prof.finish(TILE_BNECK, fl, (int)M, 4 * da.Cout, 18 * da.Cout, da.group, M * C * 2.0 + M * 4 * C * 2.0 + 18.0 * C * C * 2.0);
    }
}

}  // namespace mrcnn
