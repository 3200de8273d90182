// kernels.h — host-side launchers of the gfx950 kernels (one namespace, no torch, no templates in the API).
#pragma once
#include <stddef.h>
#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "common.h"
#include "morph_rule.h"
#include "transform_rule.h"

namespace mrcnn {

// ================================================================================================
// Box path (kernels_boxes.hip): top-k → decode → NMS, detection filtering.  -ffp-contract=off.
// ================================================================================================

// Workspace of the proposal path for a batch of images; all pointers are device memory.
struct ProposalWorkspace {
    int B = 0, A = 0, K = 0, Kpad = 0, max_keep = 0, nblk = 0, W = 0;
    uint32_t* keys = nullptr;        // [B][A]      order keys of the foreground scores
    uint32_t* hist = nullptr;        // [B][3][4096] radix-select histograms (12+12+8 bits)
    uint32_t* blockhist = nullptr;   // [B][nblk][256] per-block histogram of the last 8 bits
    uint32_t* state = nullptr;       // [B][8]      {prefix, k_remaining, threshold key, need_ties, n_gt, slot counter}
    uint64_t* cand = nullptr;        // [B][Kpad]   (~key << 32 | index), sorted ascending
    int32_t* topk_idx = nullptr;     // [B][K]      anchor index of the i-th best score
    float* boxes = nullptr;          // [B][K][4]   decoded + clipped boxes in score order
    uint64_t* nms_mask = nullptr;    // [B][K][W]   bit j of word w of row i: box 64w+j (> i) is suppressed by i
    int32_t* keep_idx = nullptr;     // [B][max_keep]
    int32_t* keep_count = nullptr;   // [B]
    static size_t bytes(int B, int A, int K, int max_keep);
    void bind(void* base, int B, int A, int K, int max_keep);
};

// ProposalLayer.evaluate for B images.  probs (B, A, 2) / deltas (B, A, 4) with batch strides in
// elements; anchors (A,4); rois out: B × max_proposals rows of `row_stride` floats (first 4 written,
// whole rows zeroed beyond the kept count — ProposalLayer.swift:181-192).
void proposal_forward(hipStream_t s, const ProposalWorkspace& ws, const float* probs, long probs_sB,
                      const float* deltas, long deltas_sB, const float* anchors, const float std4[4],
                      float nms_thr, float* rois, long rois_sB, long row_stride);

struct DetectionWorkspace {
    int B = 0, N = 0, max_det = 0, W = 0, Npad = 0;
    int32_t* count = nullptr;        // [B]        rows surviving the score/background filter
    int32_t* src = nullptr;          // [B][N]     original ROI index of filtered row k
    float* boxes = nullptr;          // [B][N][4]  refined, clipped
    float* score = nullptr;          // [B][N]
    int32_t* cls = nullptr;          // [B][N]
    uint64_t* nms_mask = nullptr;    // [B][N][W]
    int32_t* keep_idx = nullptr;     // [B][N]
    int32_t* keep_count = nullptr;   // [B]
    static size_t bytes(int B, int N, int max_det);
    void bind(void* base, int B, int N, int max_det);
};

// DetectionLayer.evaluate for B images: rois (B, N, 4) rows of roi_stride, cls6 (B, N, 6) contiguous
// rows, out: B × max_det rows of row_stride floats.
void detection_forward(hipStream_t s, const DetectionWorkspace& ws, const float* rois, long rois_sB,
                       long roi_stride, const float* cls6, long cls_sB, const float std4[4],
                       float score_thr, float nms_thr, int num_classes_hint, float* out, long out_sB,
                       long row_stride);

// ================================================================================================
// ROIAlign (kernels_roialign.hip).  -ffp-contract=off.
// ================================================================================================
struct PyramidMaps {
    const void* data[4];
    int H[4], W[4];
    long sB[4];          // batch stride in elements
    float mul[4] = {1.f, 1.f, 1.f, 1.f};   // NHWC kernel: every sample of level l is multiplied by mul[l] — exact powers of two that bring
                                           // levels stored at different split exponents to the output's (engine.h: SplitGroup)
};
// layout_nhwc = 1: maps are (B,H,W,C) and out is (B,n,P,P,C); 0: maps (B,C,H,W), out (B,n,C,P,P).
// dtype: element type of the maps and of the output (MRCNN_F16 only with layout_nhwc = 1).
void roi_align_forward(hipStream_t s, const PyramidMaps& maps, int C, int layout_nhwc, const float* rois,
                       long rois_sB, long roi_stride, int n_rois, int B, int pool, double image_w,
                       double image_h, void* out, long out_sB, long out_row_stride, int dtype,
                       int32_t* row_flags = nullptr);   // NHWC only: [B][n_rois] 1 iff every fp32 sample of the row != 0

// `.scaleFit` letterbox of an RGB8 image into an H×W canvas (content nh×nw at offset (py,px)).
void letterbox_forward(hipStream_t s, const uint8_t* src, int h, int w, uint8_t* dst, int H, int W, int nh, int nw, int py, int px);
// The same resampling fused with the mean subtraction, straight into the stem's padded staging tensor (B images of h×w).
void preprocess_scalefit_forward(hipStream_t s, const uint8_t* src, int B, int h, int w, int H, int W, int nh, int nw, int py, int px, int pad,
                                 const float mean[3], void* out, int dtype);
// One image of a mixed-size batch: where its bytes start in the buffer the kernel is given (the h×w×3 source pixels for the
// pre-processing, the pasted planes for paste_masks_source_forward) and its letterbox geometry
// (mrcnn_letterbox_geometry at the model's input size).  The table lives on the device, one entry per image.
// pitch = the distance between two source rows in PIXELS, read by the pre-processing alone: w for a whole image, the image's width
// for a window cut from it (mrcnn_maskrcnn_predict_tiles: offset = the window's origin pixel, h / w = the window's size).
struct ImageGeom {
    long long offset;
    int h, w, nh, nw, py, px;
    int pitch;
};
void preprocess_images_forward(hipStream_t s, const uint8_t* src, const ImageGeom* tab, int B, int H, int W, int pad, const float mean[3],
                               void* out, int dtype);
// Full-resolution binary instance masks from the 28×28 sigmoid masks (resize to box + threshold).
void paste_masks_forward(hipStream_t s, const float* det, long det_stride, const float* masks, int n, int S, int H, int W,
                         float thr, uint8_t* out);
// The same in every image's own frame, for a batch of images of different sizes: entry b (an ImageGeom, above) says where image
// b's `rows` planes of h×w bytes start in `out` (bytes) and how it was letterboxed.  det (batch, rows, 6) in the letterboxed H×W frame → det_src in the
// source frame (mrcnn_unletterbox_boxes' arithmetic) and the pasted planes; `boxes` is scratch of batch * rows int4,
// max_bytes = the largest rows*h*w of the batch (sizes the grid).  Two launches in all.
void paste_masks_source_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, int batch, int rows, int S,
                                int H, int W, long max_bytes, float thr, float* det_src, int4* boxes, uint8_t* out);
// COCO run-length encoding of the same planes without pasting them (mrcnn_masks_rle_source), in two steps with the capacity check
// between them.  _count: det_src and `boxes` as above, then per instance its number of runs, area and tight box (areas / bboxes may be
// nullptr) and run_offsets (batch * rows + 1 entries; the last = the runs of the whole batch).  segs (batch * rows * RLE_SEGS) and
// nruns (batch * rows) are scratch the second step reads.  _write: the run lengths of instance k at counts[run_offsets[k] ..
// run_offsets[k + 1]); counts must hold run_offsets[batch * rows] entries.
constexpr int RLE_SEGS = 16;                 // an instance's positions are walked as 16 contiguous segments, one per wave of its block
struct RleSeg { uint32_t count, last; };     // one segment: its transitions and the position of the last one
void masks_rle_count_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, int batch, int rows, int S, int H, int W,
                             float thr, float* det_src, int4* boxes, RleSeg* segs, uint32_t* nruns, long long* run_offsets, uint32_t* areas,
                             int32_t* bboxes);
void masks_rle_write_forward(hipStream_t s, const float* masks, const ImageGeom* tab, int batch, int rows, int S, float thr, const int4* boxes,
                             const RleSeg* segs, const long long* run_offsets, uint32_t* counts);
// The box-mapping launch the three entries above start with, on its own: det → det_src and the pixel boxes (batch * rows int4).
void unletterbox_boxes_forward(hipStream_t s, const float* det, const ImageGeom* tab, int batch, int rows, int H, int W, float* det_src, int4* boxes);

// ================================================================================================
// Drawing (kernels_render.hip; DetectionRenderer.swift:13-88): one launch per entry for the whole ragged batch, after the box mapping
// ================================================================================================
// Instance-id map: entry b of `tab` says where image b's h×w int16 start in `map` (byte offset).  map[y,x] = the lowest row with
// score > min_score whose pasted plane is set there, -1 for none; visible (batch * rows, may be nullptr) = the pixels each row owns.
// max_pixels = the largest h*w of the batch (sizes the grid).  det_src and boxes as in paste_masks_source_forward.
void instance_map_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, int batch, int rows, int S, int H, int W,
                          long max_pixels, float thr, float min_score, float* det_src, int4* boxes, int16_t* map, uint32_t* visible);
// Rendered overlay: srcs[b] = image b's RGB8 source (a device table of device pointers), tab[b].offset = where its h×w×3 bytes start in
// `out`.  Stroke ring of the lowest drawn row opaque, else the fill of the lowest drawn row blended with alpha/256, else the source.
void render_detections_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, const uint8_t* const* srcs, int batch,
                               int rows, int S, int H, int W, long max_pixels, float thr, float min_score, int alpha, int stroke, float* det_src,
                               int4* boxes, uint8_t* out);

// ================================================================================================
// JPEG decode behind the entropy decoder (kernels_jpeg.hip; the arithmetic is jpeg_math.h's, shared with the host definition)
// ================================================================================================
// One image of a ragged batch.  Its coefficient blocks (64 int16 each, natural order) are blocks [block0, block0 + sum of the grids) of
// the batch's coefficient array, component after component, row-major over each component's MCU-padded grid; its sample planes sit at
// comp[c].plane0 (bytes, multiple of 16) of the batch's plane buffer with a row pitch of blocks_w * 8.
struct JpegComp {
    long long block0;          // first block of the component, counted over the whole batch
    long long plane0;
    int blocks_w, blocks_h;
    int width, height;         // the component's real samples
};
struct JpegDesc {
    long long out_offset;      // byte offset of the h*w*3 RGB8 bytes in `out`
    long long block0;          // = comp[0].block0
    long long chunk0;          // first 16-pixel output chunk of the image, counted over the whole batch
    int h, w, ncomp, mode;     // mode: jpeg_math.h MODE_*
    int reserved[2];           // (keeps quant, and the next entry of a table, on 16-byte boundaries: the kernels load rows of it as uint4)
    JpegComp comp[3];
    uint16_t quant[3][64];     // per component, natural order
};
static_assert(sizeof(JpegDesc) % 16 == 0 && offsetof(JpegDesc, quant) % 16 == 0, "JpegDesc: quant rows are loaded 16 bytes at a time");
// Launch 1: dequantise + islow IDCT of every block of every component of every image -> planes.  Launch 2: chroma upsampling and
// YCbCr -> RGB per output pixel -> out + tab[b].out_offset.  total_blocks / total_chunks: the sums over the batch.
void jpeg_decode_forward(hipStream_t s, const JpegDesc* tab, int batch, const int16_t* coef, long long total_blocks, uint8_t* planes,
                         long long total_chunks, uint8_t* out);

// ================================================================================================
// JPEG encode, all of it (kernels_jpeg_enc.hip; the arithmetic and the code words are jpeg_math.h's, shared with the host definition)
// ================================================================================================
// One image of a ragged batch.  Its blocks are [block0, block0 + blocks) of the batch in SCAN order: MCU after MCU, in an MCU the
// hs * vs luma blocks row-major, then Cb, then Cr (a grey image: one block per MCU).
struct JpegEncDesc {
    const uint8_t* rgb;        // device, h*w*3, any alignment
    long long block0, blocks;
    int h, w, sampling, ncomp; // sampling: jpeg_math.h ENC_*
    int hs, vs, mcus_x, blocks_per_mcu;
    int header0, header_len;   // the file's bytes before the scan, in the batch's header blob
    int reserved[4];           // (the size stays a multiple of 16)
    uint16_t quant[2][64];     // luma, chroma; natural order
};
static_assert(sizeof(JpegEncDesc) % 16 == 0, "JpegEncDesc: a table of them keeps 16-byte alignment");
// entry[symbol] = length << 16 | code, [0] luma, [1] chroma — jpeg_enc_host.h's EncHuffman, as the device reads it
struct JpegEncHuffman {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t zigzag_of[64];     // natural index -> zigzag position
};
constexpr int JPEG_ENC_CHUNK = 128;            // bytes of unstuffed scan per stuffing thread; an image's scan starts on a chunk boundary
constexpr int JPEG_ENC_BLOCK_BYTES = 208;      // >= the 1660 bits a block can cost: DC 11 + 11, 63 x (16 + 10)
// The device buffers of one call, all but `tab`, `huff` and `headers` written by the launches.  max_chunks = the chunks the scans of all
// images can need at JPEG_ENC_BLOCK_BYTES a block; stream holds max_chunks * JPEG_ENC_CHUNK bytes (cleared by jpeg_encode_forward).
struct JpegEncBuffers {
    const JpegEncDesc* tab;
    const JpegEncHuffman* huff;
    const uint8_t* headers;
    int16_t* coef;                   // total_blocks * 64, zigzag order within a block
    uint32_t* block_bits;            // total_blocks
    unsigned long long* block_scan;  // total_blocks + 1: exclusive sum of block_bits over the whole batch
    long long* image_chunk0;         // batch + 1: first chunk of each image's scan in `stream`
    long long* image_bytes;          // batch: bytes of each image's unstuffed scan
    uint32_t* stream;                // words, most significant bit first
    uint32_t* chunk_ff;              // max_chunks: FF bytes per chunk
    unsigned long long* chunk_scan;  // max_chunks + 1
    long long* file_offsets;         // batch + 1: the result, bytes into `files`
    uint8_t* files;                  // files_capacity bytes
    long long max_chunks, files_capacity;
};
// One fill and eight launches whatever the batch: forward DCT, code lengths, their scan, the bits, FF counts, their scan, stuffing, headers + EOI.
void jpeg_encode_forward(hipStream_t s, const JpegEncBuffers& b, int batch, long long total_blocks);

// ================================================================================================
// PNG encode of label images (kernels_png.hip; the format is png_format.h's)
// ================================================================================================
// One image of a ragged batch.  Its deflate blocks (4096 raw bytes each, the last shorter) are [block0, block0 + blocks) of the batch.
struct PngDesc {
    const void* pixels;        // device; uint8 (GREY8) or int16 (INSTANCE), h*w, naturally aligned
    long long block0, blocks;
    long long n;               // raw bytes: h * (w + 1)
    int h, w;
    int header0, header_len;   // its host-built chunks (signature .. the last chunk before IDAT) in `headers`
};
static_assert(sizeof(PngDesc) % 16 == 0, "PngDesc: a table of them keeps 16-byte alignment");
// The device buffers of one call, all but `tab` and `headers` written by the launches.  files holds files_capacity bytes (a multiple of
// 4, at least the sum of png_host.h's max_file_bytes) and is cleared by png_encode_forward, as is adler.
struct PngBuffers {
    const PngDesc* tab;
    const uint8_t* headers;
    uint32_t* block_bits;            // total_blocks: header + tokens + end of block
    unsigned long long* block_scan;  // total_blocks + 1
    unsigned long long* adler;       // batch x 2: the blocks' reduced contributions to a and b
    long long* file_offsets;         // batch + 1
    uint32_t* files;                 // the files back to back, IDAT's CRC-32 left zero for the host
    long long files_capacity;
};
// Two fills and four launches whatever the batch: token bits + Adler sums, their scan + file offsets, the bits, the framing.
void png_encode_forward(hipStream_t s, const PngBuffers& b, int batch, long long total_blocks, int format, int rows);

// ================================================================================================
// Convolution family + element-wise helpers (kernels_conv.hip: the 128-row kernel; conv_dispatch.hip: which kernel runs a layer;
// kernels_elementwise.hip: the helpers)
// ================================================================================================
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2 };

struct ConvDesc {
    // element type of activations / filters / residual: MRCNN_F32 or MRCNN_F16 (fp32 accumulate)
    int dtype = MRCNN_F32;
    int out_f32 = 0;             // with MRCNN_F16: store the output(s) as fp32
    // element type of the filters; -1 = same as dtype.  (dtype F32, wdtype F16) selects the split mode:
    // fp32 tensors, each convolution as two fp16 MFMA passes over a hi/lo split of the activations.
    int wdtype = -1;
    // input NHWC (channel stride 1), arbitrary outer strides in elements
    const void* in = nullptr;
    int B = 0, H = 0, W = 0, Cin = 0;
    long in_sB = 0, in_sH = 0, in_sW = 0;
    // filter: packed [Npad][KH*KW*Cin], k contiguous (tap-major, channel-minor)
    const void* wgt = nullptr;
    // the same filters re-tiled for the halo kernel (kernels_conv_halo.hip: conv_halo_pack); nullptr = not available
    const void* wgt_halo = nullptr;
    // fp16 mode: the same filters in MFMA-fragment order for the fused bottleneck (kernels_bneck.hip: bneck_pack_frag); nullptr = not available
    const void* wgt_frag = nullptr;
    // fp16 mode, 3x3 stride-1 layers: the filters in the stream order of k_conv3x3_h (kernels_conv3x3_h.hip: conv3x3h_pack); nullptr = not available
    const void* wgt_c3h = nullptr;
    // split modes, the pointwise layers of a C = 256 stage: the filters as the chained pair's stream image (conv_pack.h: pack_chain_stream); nullptr = not available
    const void* wgt_stream = nullptr;
    int prefer_c3h = 0;         // run on that kernel even without a fused head (the engine's A/B of the head fusion: "conv_c3h" 3)
    int KH = 1, KW = 1, stride = 1, padH = 0, padW = 0;
    // epilogue: y = act(acc*scale[n] + shift[n] + residual)
    const float* scale = nullptr;
    const float* shift = nullptr;
    // `res` MAY ALIAS `out` (the engine writes every bottleneck block's output in place over its shortcut).  Contract of every
    // epilogue form: the residual element at an address is loaded by the SAME thread that stores the output element there, and
    // before that store; no epilogue may prefetch residual elements another thread (or a later pass) stores over.  Pinned by
    // tests/test_gpu_conv_kernels.py::test_every_epilogue_is_safe_in_place_over_its_residual.
    const void* res = nullptr;
    long res_sB = 0, res_sH = 0, res_sW = 0;
    int res_shift = 0;           // residual read at (oh >> res_shift, ow >> res_shift): nearest 2× upsample when 1
    int act = ACT_NONE;
    // output NHWC: address = b*out_sB + (oh*OW+ow)*out_sP + n  (rows of the image contiguous)
    void* out = nullptr;
    int OH = 0, OW = 0, Cout = 0, Npad = 0;
    long out_sB = 0, out_sP = 0;
    // optional second output: columns >= n_split go to out2 (column n - n_split)
    void* out2 = nullptr;
    int n_split = 0;
    long out2_sB = 0, out2_sP = 0;
    // transposed-conv 2x2 stride 2 scatter: column n = q*Cout + co, q = dy*2+dx → pixel (2oh+dy, 2ow+dx)
    int deconv2 = 0;
    long out_sH = 0, out_sW = 0;  // only used when deconv2
    // algorithmic reduction length per output (defaults to KH*KW*Cin; conv1 pads 147 → 224)
    int algo_k = 0;
    // profile bookkeeping only: 1 = a backbone convolution (conv1, res2..res5), 0 = anything else (FPN, RPN, heads)
    int group = 0;
    // deconv2 only — selected-class dot instead of the store (the mask head's last two layers fused): for input image
    // (= ROI row) b with class sel_cid[b] >= 0, every output pixel P contributes
    //   sel_partial[(b * 4*OH*OW + P) * (Cout/128) + h] = Σ_{co in 128-channel part h} y[P][co] * sel_w[sel_cid[b]][co]
    // (y = the activated output, rounded to fp16 first when dtype is MRCNN_F16); nothing is written to `out`.
    const float* sel_w = nullptr;
    const int32_t* sel_cid = nullptr;
    float* sel_partial = nullptr;
    // halo kernel only — a 1x1 head fused into this layer's epilogue (the RPN's class / box heads on the shared 3x3 layer): the
    // layer's own output is not stored; head_out gets head columns [0, head_split), head_out2 the columns [head_split, head_cols),
    // each + head_bias.  head_w = conv_halo_pack_head of the [32][Cout] head filters.  conv_halo_head_eligible says whether the
    // layer can run fused (a property of its geometry only); conv_forward fails loudly when it cannot.
    const void* head_w = nullptr;
    const float* head_bias = nullptr;
    float* head_out = nullptr; float* head_out2 = nullptr;
    long head_out_sB = 0, head_out_sP = 0, head_out2_sB = 0, head_out2_sP = 0;
    int head_split = 0, head_cols = 0;
    float head_mul = 1.f;        // the head's sums are multiplied by this before the bias (2^-e of this layer's output group: exact)
};

// Live per-kernel profile of the conv family: when a profiler is active on the calling thread every
// conv_forward launch is bracketed by HIP events on its own stream; collect() (after the stream
// has been synchronised) folds the elapsed times into per-tile-shape totals.
// The tile classes of the profile (the index of ConvProfile::by_tile, the `tile` of a shape key; bench.py reads the numbers)
enum ConvTileClass {
    TILE_128x128 = 0,
    TILE_128x64 = 1,
    TILE_128x32 = 2,
    TILE_128x128_4WAVE = 3,      // 128x128 run by 4 waves of 32x128 (split modes, long K)
    TILE_PP_256x256 = 4,         // 256x256 ping-pong
    TILE_HALO = 5,               // persistent halo tiles (3x3 stride 1, split modes)
    TILE_HALO_TAIL = 6,          // halo tiles with the fused bottleneck tail (3x3 + 1x1)
    TILE_BNECK = 7,              // a whole identity bottleneck of the fp16 mode in one launch (kernels_bneck.hip; flops of its three layers)
    TILE_C3H = 8,                // 16 x 16 halo tiles x 256 columns of the fp16 mode's 3x3 layers (kernels_conv3x3_h.hip)
    TILE_CLASSES
};
struct ConvProfile {
    struct Slot { long launches = 0; double ms = 0, flops = 0, bytes = 0; };       // bytes: ALGORITHMIC bytes (conv_algorithmic_bytes: every operand once)
    Slot by_tile[TILE_CLASSES];      // per ConvTileClass
    std::vector<hipEvent_t> pool;
    struct Shape { int M, N, K, tile; bool operator<(const Shape& o) const { return std::tie(M, N, K, tile) < std::tie(o.M, o.N, o.K, o.tile); } };
    std::map<Shape, Slot> by_shape;  // per GEMM shape (M = images·OH·OW, N = output columns, K = taps·Cin)
    struct Pending { int tile; double flops; int e0, e1; Shape shape; int group = 0; double bytes = 0; };
    Slot by_group[2];                // ConvDesc::group: 0 = everything else, 1 = the backbone convolutions (C1..C5: north_star's roofline target is worded on them)
    std::vector<Pending> pending;
    int used = 0;
    bool active = false;
    void reset();
    void collect();
    ~ConvProfile();
};
void conv_set_profiler(ConvProfile* p);   // thread-local; nullptr disables
// One-time per-process set-up; idempotent, called at model / layer creation.
void boxes_one_time_init();
// While set (thread-local), every conv launch ORs 1 into *device_flag when one of its outputs leaves the fp16
// range (|v| >= 65504, inf or NaN): the watchdog of the fp16-MFMA modes, whose next layer reads it through fp16.
void conv_set_range_flag(int* device_flag);
// Device scratch of the convolution family (the partial sums + tile counters of shared-tile K chunks, the fused bottleneck tail's
// parking buffer).  OWNED by whoever launches — a Model (allocated at load, freed with it), a stand-alone test entry (for the call) —
// and handed to the launches of the calling thread like the range flag.  Without one the kernels that need it are not chosen
// (a chunked layer sums its chunks in one block: the same bits), so nothing is ever allocated behind a caller's back or inside a
// stream capture, and nothing outlives its owner.
struct ConvScratch {
    DevBuf ks_buf, ks_cnt, park;
    void alloc();            // synchronous; call outside any stream capture
    static size_t ks_bytes();
};
void conv_set_scratch(ConvScratch* c);    // thread-local; nullptr = none
// Picks the tile shape from Cout; returns the N tile it will use so that callers can pad weights.
int conv_n_tile(int Cout);
// sc != nullptr: `sc` is the 1x1 convolution whose output is d's residual (a ResNet stage's shortcut): computed inside d's launch where the pair
// qualifies (bit-identical to the two launches; the shortcut tensor is then not written), as its own launch before d otherwise
void conv_forward(hipStream_t s, const ConvDesc& d, const ConvDesc* sc = nullptr);
// Halo kernel (kernels_conv_halo.hip): 3x3 stride-1 layers of the split modes.  conv_halo_pack re-tiles [Npad][9][Cin] fp16
// filters (device) into its granule layout; conv_halo_eligible says whether a layer can run on it (a property of the layer's
// geometry and mode only — never of the batch: the K order of the kernel differs from the 128-row kernel's).
struct ConvArgs;
void conv_halo_pack(hipStream_t s, const void* wgt_std, int Npad, int Cin, DevBuf& out, int taps = 9);
void conv_halo_pack_head(hipStream_t s, const void* wgt_std, int Npad, int Cin, DevBuf& out);
bool conv_halo_eligible(const ConvDesc& d);
bool conv_halo_head_eligible(const ConvDesc& d);
bool conv_halo_enabled();                   // the run-time switch mrcnn_debug_set("conv_halo") / MRCNN_HALO
bool conv_halo_packable(int KH, int KW, int Cin, int Npad);   // the filter shapes conv_halo_eligible can accept (re-tile only those)
int conv_halo_forward(hipStream_t s, ConvArgs a, const ConvDesc& d, int parts, int n_cus, const ConvArgs* tail = nullptr, const void* tail_w = nullptr);
bool conv_halo_tail_packable(int KH, int KW, int Cin, int Npad);       // the 1x1 filters the fused bottleneck tail accepts (re-tiled with one tap)
bool conv_halo_tail_geometry_ok(int H, int W);                          // ... and the 3x3 tile geometries it is instantiated for
// A ResNet bottleneck's tail — d3: the 3x3 `branch2b` (halo-eligible, 256 output columns, ReLU), d1: the 1x1 `branch2c` that reads
// d3's output (256 -> 1024, + shortcut, ReLU; d1.wgt_halo = its filters re-tiled with one tap) — as ONE persistent launch in which the
// 256-column tensor between them never exists (kernels_conv_halo.hip: TAIL).  Bit-identical to conv_forward(d3); conv_forward(d1),
// which is what runs when the pair does not qualify, the grid would not fill the chip, or mrcnn_debug_set("conv_tail", 0).
bool conv_tail_fusable(const ConvDesc& d3, const ConvDesc& d1);
int conv_sel_part_cols();       // selected-class mode: output columns per partial sum the next conv_forward will leave (64: wave-private form, 128: block-staged)
void conv_forward_tail(hipStream_t s, const ConvDesc& d3, const ConvDesc& d1, const ConvDesc* sc = nullptr, const ConvDesc* q = nullptr);      // sc: d1's shortcut convolution (conv_forward); q: the layer chained behind d1 (conv_forward_chain)
// Chained pair of the split modes (kernels_conv_chain.hip): dP = a bottleneck's branch2c (1x1, C -> 4C, residual or fused shortcut sc, ReLU) and
// dQ = the NEXT block's branch2a (1x1, 4C -> C, ReLU) reading dP's output, C = 64 | 128 | 256 — ONE launch: dP's output is stored and dQ is computed from
// the tile while it is on chip.  BIT-IDENTICAL to conv_forward(dP, sc); conv_forward(dQ), which run where the pair does not qualify, the grid
// under-fills the chip, C = 128 (measured slower: DESIGN.md section 3.1r), or behind mrcnn_debug_set("conv_chain", 0) ("conv_chain" 2: every
// pair conv_chain_fusable accepts, at every grid size).  conv_chain_fusable says what the kernel can run, not what the policy chooses.
// C = 256 (C4) has a knob of its own, "conv_chain4" (0 never, 1 by policy, 2 at every grid size), runs identity pairs only — a dP that carries the
// stage's shortcut, fused or as a tensor, is never chained — and needs both layers' stream images (ConvDesc::wgt_stream).
bool conv_chain_fusable(const ConvDesc& dP, const ConvDesc& dQ, const ConvDesc* sc = nullptr);
void conv_forward_chain(hipStream_t s, const ConvDesc& dP, const ConvDesc& dQ, const ConvDesc* sc = nullptr);

// An identity ResNet bottleneck of the fp16 mode — da: the 1x1 `branch2a` (4C -> C, ReLU), db: the 3x3 `branch2b` reading da's output
// (C -> C, ReLU), dc: the 1x1 `branch2c` reading db's output (C -> 4C, + shortcut = da's input, ReLU), C in {64, 128, 256} — as ONE
// persistent launch (kernels_bneck.hip): the two mid tensors never leave the chip.  BIT-IDENTICAL to conv_forward(da); conv_forward(db);
// conv_forward(dc), which is what conv_bneck_forward runs when the triple does not qualify or mrcnn_debug_set("conv_bneck", 0).  The fused
// form needs dc.out != da.in (a tile reads halo pixels its neighbours own); whether a triple qualifies is a property of the layers'
// geometry only, never of the batch.
bool conv_bneck_fusable(const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc);
// The stage-ENTRY block of C2 in the fp16 mode (res2a: stride 1, 64 -> 64 -> 64 -> 256, shortcut = the 1x1 convolution ds = `branch1` of the
// block's input, whose output is dc's residual) as one launch of the same kernel (FIRST form): bit-identical to conv_forward(da);
// conv_forward(ds); conv_forward(db); conv_forward(dc), which run when the block does not qualify / the grid under-fills the chip / "conv_bneck" 0.
bool conv_bneck_first_fusable(const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc, const ConvDesc& ds);
void conv_bneck_first_forward(hipStream_t s, const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc, const ConvDesc& ds);
bool conv_bneck_enabled();
void conv_bneck_forward(hipStream_t s, const ConvDesc& da, const ConvDesc& db, const ConvDesc& dc);
bool bneck_geometry_ok(int C, int H, int W);
// w2f / w3f: W2 / W3 in MFMA-fragment order (bneck_pack_frag) — used by the C = 256 form, whose waves stream their filter fragments
// straight from L2 into registers; nullptr selects the form with every operand staged through LDS
void bneck_launch(hipStream_t s, int C, const void* x, void* y, int B, int H, int W, const void* w1, const void* w2, const void* w3,
                  const float* s1, const float* h1, const float* s2, const float* h2, const float* s3, const float* h3, int* range_flag, int n_cus,
                  const void* w2f = nullptr, const void* w3f = nullptr, const void* w1f = nullptr,
                  const void* ws = nullptr, const float* ss = nullptr, const float* hs = nullptr);      // ws / ss / hs: the stage-entry form (C = 64)
// The identity blocks of a C = 256 stage (C4) as ONE launch — kernels_bneck.hip, STAGE form: a tile's block l starts when its <= 9 neighbour
// tiles have published block l - 1 (per-tile counters `done`, device-scope stores / loads), no launch gap or drain between blocks; BIT-IDENTICAL
// to nlayers calls of bneck_launch.  layers_dev: nlayers records of bneck_layer_record_bytes() bytes written by bneck_layer_record (host) and
// copied to the device; pp0 = the stage's input, pp1 = its ping-pong partner (result in pp[nlayers & 1]); done: >= B * tiles counters.
// range_flag (required): bit 0 as everywhere, bit 1 = a tile waited ~0.1 s for a neighbour (the grid was not resident as a whole): results invalid.
void bneck_stage_launch(hipStream_t s, const void* layers_dev, int nlayers, void* pp0, void* pp1, int B, int H, int W, unsigned* done, int* range_flag, int n_cus);
size_t bneck_layer_record_bytes();
void bneck_layer_record(void* dst, const void* w1f, const void* w2f, const void* w3f, const float* s1, const float* h1, const float* s2, const float* h2,
                        const float* s3, const float* h3);
struct BneckTriple { ConvDesc a, b, c; };
// conv_bneck_forward over the consecutive identity blocks of a stage: ONE launch where every block takes the fragment-streaming form, the grid
// fills the chip and mrcnn_debug_set("conv_bneck_stage", 1) (opt-in: measured equal); the per-block launches otherwise.  layers_dev / done as above (owned by the caller).
void conv_bneck_stage_forward(hipStream_t s, const BneckTriple* blocks, int n, const void* layers_dev, unsigned* done);
// [N][K] fp16 filters (K contiguous; N % 32 == 0, K % 16 == 0) -> 1-KB granules [N/32][K/16][lane 0..63][8]: lane (l31, kk) of granule (nt, kg)
// holds filter row 32 nt + l31, k = 16 kg + 8 kk .. + 7 — the first MFMA operand of v_mfma_f32_32x32x16_f16, one coalesced 16-B load per lane
void bneck_pack_frag(hipStream_t s, const void* wgt_std, int N, int K, DevBuf& out);
bool bneck_frag_wanted(int KH, int KW, int Cin, int Cout);      // the filter shapes the C = 256 form reads in fragment order

// The 3x3 stride-1 'same' layers of the fp16 mode with 256 | 512 output columns (kernels_conv3x3_h.hip): 16 x 16 halo tiles resident in LDS per
// 64-channel block, filter fragments streamed into registers, K order (channel block, tap, group) — its own: whether a layer runs here is
// decided by the layer alone (conv3x3h_eligible), never by the batch.  mrcnn_debug_set("conv_c3h", 0) sends such layers back to the
// 128-row / ping-pong kernels (their tap-major order: results differ by summation noise).
void conv3x3h_pack(hipStream_t s, const void* wgt_std, int N, int Cin, DevBuf& out);
bool conv3x3h_packable(int KH, int KW, int Cin, int Cout, int Npad);
bool conv3x3h_eligible(const ConvDesc& d);
void conv3x3h_launch(hipStream_t s, const ConvDesc& d, int* range_flag, int n_cus);
int conv_c3h_mode();                        // mrcnn_debug_set("conv_c3h") / MRCNN_C3H: 0 never | 1 where the RPN heads ride along (default) | 2 every eligible layer | 3 as 1 with the heads as their own launch

// The stem in the split modes and the fp16 mode (kernels_conv_stem.hip): conv1 — described by d exactly as for conv_forward (7 row taps of 32 "channels"
// on the zero-padded NHWC4 input, 64 output columns, ReLU) — and the 3x3 stride-2 'same' max-pool behind it in ONE persistent launch;
// conv1's output tensor is neither written nor read.  pooled: (B, PH, PW, 64) fp32.  Bit-identical to conv_forward(d) +
// maxpool3x3s2_forward.  conv_stem_eligible: whether d is that layer in a split mode or the fp16 mode (a property of the layer, not of the batch);
// mrcnn_debug_set("conv_stem", 0) sends callers back to the two launches.
bool conv_stem_eligible(const ConvDesc& d);
bool conv_stem_enabled();
void conv_stem_forward(hipStream_t s, const ConvDesc& d, void* pooled, int PH, int PW);
void conv_stem_launch(hipStream_t s, const void* in, int B, int Hp, int Wp, const void* wgt, const float* scale, const float* shift, int CH, int CW,
                      void* out, int PH, int PW, int parts, int* range_flag, int n_cus, bool compact = true);

// uint8 RGB (B,H,W,3) → fp32 (B, H+2*pad, W+2*pad, 4) minus mean, zero border, channel 3 = 0.
void preprocess_forward(hipStream_t s, const uint8_t* rgb, int B, int H, int W, int pad, const float mean[3],
                        void* out, int dtype);   // fp32 → NHWC4, fp16 → NHWC8
// 3×3 stride-2 max pool, Keras 'same' (window clipped at the bottom/right edge). NHWC, C % 4 == 0.
void maxpool3x3s2_forward(hipStream_t s, const void* in, int B, int H, int W, int C, void* out, int OH, int OW, int dtype);
// softmax over consecutive pairs: logits (n,2) → probs (n,2)
void softmax_pairs_forward(hipStream_t s, const float* logits, float* probs, long n_pairs);
// row softmax: logits rows of ld floats, first nc columns → probs (n, nc) contiguous
void softmax_rows_forward(hipStream_t s, const float* logits, long ld, int nc, long n, float* probs);
// copy bbox columns: src rows of ld floats starting at column c0, ncols columns → dst (n, ncols)
void copy_columns_forward(hipStream_t s, const float* src, long ld, int c0, int ncols, long n, float* dst);
// TimeDistributedClassifierLayer post-processing: probs (n,nc), bbox (n,nc*4) → rows (dy,dx,dh,dw,id,score)
void classifier_postprocess_forward(hipStream_t s, const float* probs, const float* bbox, int nc, long n,
                                    float* out, long out_row_stride);
// layout changes between Core ML's CHW and the engine's HWC
void nchw_to_nhwc_forward(hipStream_t s, const float* in, long n, int C, int H, int W, void* out, int dtype);
void nhwc_to_nchw_forward(hipStream_t s, const float* in, long n, int C, int H, int W, float* out);
// strided row gather: dst[i][0..len) = src[i*src_stride .. +len)
void copy_rows_forward(hipStream_t s, const float* src, long src_stride, long n, long len, float* dst, long dst_stride);

// TimeDistributedMaskLayer pieces -----------------------------------------------------------------
struct MaskSelectWorkspace {
    int32_t* flags = nullptr;      // [B][D] row is all-nonzero
    int32_t* mapping = nullptr;    // [B][D] compact index → row
    int32_t* kept = nullptr;       // [B]
    int32_t* sel_cid = nullptr;    // [B][D] class per row for the fused tail (mask_select_classes), -1 = not written
    int ld = 0;                    // rows per image of the three [B][D] arrays; 0 = the D of each call.  Set it where the predicate runs on
                                   // fewer rows than the select pads (the stand-alone layer's D feature rows under det_count detections) in a batch.
};
// flags/mapping of MultiArrayBatchProvider(removeZeros:true): pooled (B, D, row_len) contiguous rows.
// pooled == nullptr: ws.flags already holds the predicate (written by roi_align_forward's row_flags from the fp32
// samples — the fused engine path, also in fp16 mode where the stored rows are rounded); only the compaction runs.
void mask_valid_rows_forward(hipStream_t s, const void* pooled, long pooled_sB, long row_stride, long row_len,
                             int D, int B, const MaskSelectWorkspace& ws, int dtype);
// feat (B, D, HW, C) = ReLU(deconv) NHWC; w (nc, C), bias (nc); detections rows det_stride;
// out rows out_stride (>= HW).  Writes exactly what TimeDistributedMaskLayer.swift:58-89 writes.
void mask_select_forward(hipStream_t s, const void* feat, long feat_sB, int HW, int C, const float* w,
                         const float* bias, int nc, const float* det, long det_sB, long det_stride, int D, int B,
                         const MaskSelectWorkspace& ws, float* out, long out_sB, long out_stride, int dtype);
// The same result from the partial dots a deconv2 convolution in selected-class mode left (ConvDesc::sel_partial):
//   mask_select_classes: sel_cid[b*D + row] = the class the layer would use for that row, -1 for rows it does not write;
//   mask_select_from_partials: sigmoid(Σ_h partial[...][h] + bias[class]) into the rows the layer writes, zero padding as above.
void mask_select_classes(hipStream_t s, const float* det, long det_sB, long det_stride, int D, int B, int nc,
                         const MaskSelectWorkspace& ws, int32_t* sel_cid);     // sel_cid = ws.sel_cid in the engine
void mask_select_from_partials(hipStream_t s, const float* partial, int parts, int HW, const float* bias, int nc, const float* det,
                               long det_sB, long det_stride, int D, int B, const MaskSelectWorkspace& ws, float* out, long out_sB,
                               long out_stride);
// Variant for precomputed per-class masks (n_kept-compacted or in-place), used by the stand-alone layer:
// masks (B, D, nc, HW) in place (row r of the batch = detection r).
void mask_select_from_full_forward(hipStream_t s, const float* masks, long masks_sB, int HW, int nc,
                                   const float* det, long det_sB, long det_stride, int D, int B,
                                   const MaskSelectWorkspace& ws, float* out, long out_sB, long out_stride);

// ================================================================================================
// COCO scoring (kernels_coco.hip): RLE x RLE intersection, box IoU, COCOeval's greedy matching.  -ffp-contract=off.
// ================================================================================================
using IouGroup = mrcnn_iou_group;          // one image: detections [d0, d1) x ground truths [g0, g1), block at out_offset
using MatchGroup = mrcnn_match_group;      // one (image, category): ranges of the flat detection / ground-truth lists
// Per RLE k (counts[run_offsets[k] .. run_offsets[k+1])): pre_b = exclusive prefix of the counts, pre_o = exclusive prefix of the odd
// (ones) runs, both indexed like counts (either may be nullptr); totals[k] = the pixels, areas[k] = the set pixels.  One block per RLE.
// extent[k] (may be nullptr) = the positions of the first and the last set pixel, (0xffffffff, 0) for an empty mask.  kernels_rle_prefix.hip.
void rle_prefix_forward(hipStream_t s, const uint32_t* counts, const long long* run_offsets, long n_rle, uint32_t* pre_b, uint32_t* pre_o,
                        unsigned long long* totals, uint32_t* areas, uint2* extent = nullptr);

// ================================================================================================
// Drawing run-length masks (kernels_rle_draw.hip): planes, instance maps and overlays of a ragged batch from an RLE set.
// ================================================================================================
// One RLE after rle_draw_prepare: its runs, the positions of its first and last set pixel, its row's pixel box, whether it is drawn
struct RleDrawRec { long long r0; int nruns; uint32_t first, last; int y1, x1, y2, x2; int drawn; };
struct RleDrawJob {
    const RleDrawRec* rec;            // n_images * slots
    const uint32_t* pre_b;            // rle_prefix_forward's B, indexed like counts
    const ImageGeom* tab;             // n_images: h, w and the byte offset of the image's output; the rest is not read
    int n_images, slots;
    int max_h, max_w;                 // the largest sides of the batch: the grid
};
// rec[k] from the prefix pass and (det != nullptr) the detection rows; det == nullptr draws every RLE (the decode).  *bad (device, one
// word) = the lowest k whose total is not its plane's h*w, ~0 if all are right: the caller reads it back before it draws.
void rle_draw_prepare(hipStream_t s, const long long* run_offsets, const unsigned long long* totals, const uint2* extent, const float* det,
                      float min_score, const RleDrawJob& job, RleDrawRec* rec, unsigned long long* bad);
void rle_decode_forward(hipStream_t s, const RleDrawJob& job, uint8_t* out);
void instance_map_rle_forward(hipStream_t s, const RleDrawJob& job, int16_t* map, uint32_t* visible);
void render_detections_rle_forward(hipStream_t s, const RleDrawJob& job, const uint8_t* const* srcs, int alpha, int stroke, uint8_t* out);

// ================================================================================================
// Morphology on run-length masks (kernels_rle_morph.hip; the rule is morph_rule.h).  All tables are device arrays.
// ================================================================================================
constexpr int MORPH_TILE = 4096;      // words of one word row a block stages: C + 2r with C >= 2048 output columns at the largest radius
static_assert(MORPH_TILE >= 2 * MRCNN_MORPH_MAX_RADIUS + 2048, "a tile holds its halo at the largest radius");
// One RLE after the boxes were read back: its runs, plane and radius, the tight box of its set pixels, the box its result lies in
// (`work`: `words` word rows of work.x2 - work.x1 words, 32 rows per word), and where its words, columns and tiles start in the call's
struct MorphRec { long long r0, word0, col0, tile0; MorphBox tight, work; int h, w, r, nruns, words, pad; };
struct MorphJob {
    const MorphRec* rec; int n; int op;
    long long cols, tiles;            // the columns of all boxes; the tiles: per RLE words * ceil(columns / (MORPH_TILE - 2r))
    const uint32_t* counts;
    const uint32_t* pre_b;            // rle_prefix_forward's B, indexed like counts
    uint32_t *va, *vb;                // two bit boxes per RLE: the vertical half's result (and the mask's own bits for BOUNDARY), the result
};
// tight[k] from the runs and rle_prefix_forward's totals and extent; *bad (device, one word) = the lowest k whose total is not its
// plane's h*w, ~0 if all are right: the caller reads both back before anything else is sized or launched
void rle_morph_boxes_forward(hipStream_t s, const uint32_t* counts, const uint32_t* pre_b, const long long* run_offsets, const int32_t* heights,
                             const int32_t* widths, const unsigned long long* totals, const uint2* extent, long n, MorphBox* tight,
                             unsigned long long* bad);
// the vertical and the horizontal half: job.vb holds the result's bits
void rle_morph_forward(hipStream_t s, const MorphJob& job);
// the encoder's two passes on those bits, as masks_rle_count_forward / masks_rle_write_forward run them (segs: n * RLE_SEGS, nruns: n)
void rle_morph_count_forward(hipStream_t s, const MorphJob& job, RleSeg* segs, uint32_t* nruns, long long* run_offsets, uint32_t* areas, int32_t* bboxes);
void rle_morph_write_forward(hipStream_t s, const MorphJob& job, const RleSeg* segs, const long long* run_offsets, uint32_t* counts);

// ================================================================================================
// The set algebra of run-length masks (kernels_rle_combine.hip; the rule is combine_rule.h).  All tables are device arrays.
// ================================================================================================
constexpr int COMBINE_PASS_WORDS = 32;                           // word rows a thread keeps in LDS: 1024 rows of a box per pass
// one member of a group: its runs and the tight box of its set pixels (an empty mask: (0, 0, 0, 0))
struct CombineMember { long long r0; int nruns; MorphBox tight; int pad; };
struct CombineJob {
    const MorphRec* rec; int n;       // one per group, laid out as mrcnn_rle_morph lays its bit boxes out: work, words, word0, col0, h and w (the rest 0)
    const long long* member0;         // n + 1: group g owns members[member0[g] .. member0[g+1]), the first one first
    const CombineMember* members;
    int op;
    long long cols;                   // the columns of all work boxes
    const uint32_t* counts;
    const uint32_t* pre_b;            // rle_prefix_forward's B, indexed like counts
    uint32_t* bits;                   // the groups' bit boxes: every word of them is written
};
// the fold of every group's members into its bit box; rle_morph_count_forward / rle_morph_write_forward encode the boxes (MorphJob.vb = bits)
void rle_combine_forward(hipStream_t s, const CombineJob& job);

// ================================================================================================
// Moving run-length masks to another pixel grid (kernels_rle_transform.hip; the rule is transform_rule.h).  All tables are device arrays.
// ================================================================================================
constexpr int XF_PASS_WORDS = 32;                                // word rows a thread keeps in LDS: 1024 rows of a box per pass
// the source of one output RLE: its runs, its plane, the tight box of its set pixels (an empty mask: (0, 0, 0, 0)) and the record
struct XfSource { long long r0; int nruns, h, w, pad; MorphBox tight; XfMap map; };
struct XfJob {
    const MorphRec* rec; int n;       // one per RLE, laid out as mrcnn_rle_morph lays its bit boxes out: work, words, word0, col0, and h and w of the OUTPUT plane
    const XfSource* src;              // n
    long long cols;                   // the columns of all work boxes
    const uint32_t* counts;
    const uint32_t* pre_b;            // rle_prefix_forward's B, indexed like counts
    uint32_t* bits;                   // the bit boxes: every word of them is written
};
// every source read through its record into its bit box; rle_morph_count_forward / rle_morph_write_forward encode the boxes (MorphJob.vb = bits)
void rle_transform_forward(hipStream_t s, const XfJob& job);

// ================================================================================================
// Connected components of run-length masks (kernels_rle_components.hip; the rule is components_rule.h).  All tables are device arrays.
// ================================================================================================
// the set: heights, widths and rle_prefix_forward's totals per RLE, its B per run
struct CompSet {
    const uint32_t* counts; const uint32_t* pre_b; const long long* run_offsets;
    const int32_t* heights; const int32_t* widths; const unsigned long long* totals;
    int n, connectivity, of;
};
// The pieces, in column-major order RLE after RLE: positions [pa, pb) (x*h + y) inside one column, the RLE, the union-find parents,
// and after the labelling the root (the component's lowest piece) and the component's number in the whole set
struct CompPieces { long long n; uint32_t *pa, *pb; int32_t* rle; uint32_t *parent, *root, *comp; };
struct CompAcc { uint32_t* area; int32_t *x1, *y1, *x2, *y2; uint32_t* flag; };         // per component, while it is measured
// one group of the writer's sequence per output RLE: its places, its parent RLE, what k_cc_groups and k_cc_runs find
struct CompGroups { long long n; long long *begin, *end; int32_t* rle; uint32_t *lead, *nruns, *area; int32_t *x1, *y1, *x2, *y2; };
// the selection: keep per component; SPLIT adds the sorted order, the components' first places and the kept components' output index
struct CompSelect { const uint8_t* keep; long long n_comps; const uint32_t* order; const long long* comp_first; const unsigned long long* out_index; };
// run_cnt[j] = the pieces run run_offsets[0] + j owns, run_start = its exclusive prefix (runs + 1); *bad = the lowest RLE with a wrong total, ~0 if none
void rle_components_count_forward(hipStream_t s, const CompSet& S, long long runs, uint32_t* run_cnt, unsigned long long* run_start, unsigned long long* bad);
// pieces, links, roots and numbers: piece0 (n + 1), is_root (pieces), comp_start (pieces + 1), comp_rle (pieces at most), comp_offsets (n + 1)
void rle_components_label_forward(hipStream_t s, const CompSet& S, long long runs, const unsigned long long* run_start, const CompPieces& P,
                                  long long* piece0, uint32_t* is_root, unsigned long long* comp_start, int32_t* comp_rle, long long* comp_offsets);
void rle_components_measure_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompAcc& acc, long long n_comps, uint32_t* areas,
                                    int32_t* bboxes, uint8_t* flags);
// SPLIT's order: keys holds rle_components_sort_padded(pieces) entries, order pieces, comp_first n_comps + 1
long long rle_components_sort_padded(long long n_pieces);
void rle_components_sort_forward(hipStream_t s, const CompPieces& P, long long n_comps, unsigned long long* keys, uint32_t* order, long long* comp_first);
// flag[c] = keep[c] != 0 and its exclusive prefix out_index (n_comps + 1): out_index[n_comps] components are kept
void rle_components_keep_forward(hipStream_t s, const uint8_t* keep, long long n_comps, uint32_t* flag, unsigned long long* out_index);
// the groups (q.order: SPLIT's, else MERGE's), the boundaries each place gives (bcnt, bpos: pieces + 1), out_parent (may be nullptr
// for MERGE) and out_run_offsets (G.n + 1)
void rle_components_groups_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompSelect& q, const long long* piece0,
                                   const int32_t* comp_rle, const CompGroups& G, uint32_t* bcnt, unsigned long long* bpos, long long* out_parent,
                                   long long* out_run_offsets);
// the boundaries (bnd: bpos[pieces] entries), then the runs (counts may be nullptr: only measured) and the optional areas and boxes
void rle_components_write_forward(hipStream_t s, const CompSet& S, const CompPieces& P, const CompSelect& q, const CompGroups& G,
                                  const unsigned long long* bpos, uint32_t* bnd, const long long* out_run_offsets, long long total_runs, uint32_t* counts,
                                  uint32_t* areas, int32_t* bboxes);

// inter / iou of every pair of every group.  block_starts (n_groups + 1, device): prefix of ceil(nd / 4) * ng per group = the grid.
// The caller has checked that the two RLEs of every pair have the same total.  inter / iou may be nullptr.
void rle_iou_forward(hipStream_t s, const uint32_t* d_b, const long long* d_off, const unsigned long long* d_total, const uint32_t* d_area,
                     const uint32_t* g_b, const uint32_t* g_o, const long long* g_off, const uint32_t* g_area, const uint8_t* g_crowd,
                     const IouGroup* groups, const long long* block_starts, int n_groups, long long n_blocks, uint32_t* inter, double* iou);
// pair_starts (n_groups + 1, device): prefix of nd * ng per group; one thread per pair
void box_iou_xywh_forward(hipStream_t s, const double* db, const double* gb, const uint8_t* g_crowd, const IouGroup* groups,
                          const long long* pair_starts, int n_groups, long long n_pairs, double* iou);
// one wave per (group, area range, threshold); outputs laid out as mrcnn_coco_match documents
void coco_match_forward(hipStream_t s, const double* iou, const MatchGroup* groups, int n_groups, const int32_t* dt_idx, const double* dt_area,
                        const int32_t* gt_idx, const double* gt_area, const uint8_t* gt_crowd, const double* ranges, int A, const double* thrs, int T,
                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match);

// Polygon ground truth -> RLE (mrcnn_rle_from_polygons_batch; the arithmetic is poly_device.h).  All tables are device arrays.
// An EDGE is a point of the concatenated point list together with its successor in its polygon; its toggles are the pixel-column
// centres it crosses.  The toggles of an annotation are contiguous in edge order: toggle q of the batch belongs to the edge e with
// edge_start[e] <= q < edge_start[e + 1].
struct PolyRec { long long pt0; int npts, ann; };                 // one polygon: its points [pt0, pt0 + npts) and its annotation
struct PolyAnn { long long pt0, pt1; int poly0, h, w, pad; };     // one annotation: its points, its first polygon, its plane
struct PolyBig { long long ann, offset, padded; };               // an annotation on the global sort path: its slice of the scratch, a power of two
constexpr int POLY_LDS_TOGGLES = MRCNN_POLY_LDS_TOGGLES;                           // toggles an annotation may have to be sorted in LDS (8 B keys + 4 B coverage = 48 KiB)
// edge_cnt[e] = the toggles of edge e, edge_start = its exclusive prefix (n_pts + 1), tog_off[k] = edge_start[anns[k].pt0] (n_anns + 1)
void poly_count_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns, long n_pts, long n_anns,
                        uint32_t* edge_cnt, long long* edge_start, long long* tog_off);
// Annotations of at most POLY_LDS_TOGGLES toggles, one block each: generate, sort per polygon, pair, sort per annotation, unite.  The run
// boundaries of annotation k land at bnd[tog_off[k] ..], their number in nb[k]; nruns[k], areas[k], bboxes[4k ..] (may be nullptr) follow.
void poly_encode_lds_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns, long n_anns,
                             const long long* edge_start, uint32_t* bnd, uint32_t* nb, uint32_t* nruns, uint32_t* areas, int32_t* bboxes);
// The same for the annotations listed in `big` (host copy: h_big), sorted in global memory: keys (8 B) and cov (4 B) hold the sum of the
// padded sizes.  The number of launches grows with the logarithm of the largest padded size, not with the number of annotations.
void poly_encode_big_forward(hipStream_t s, const double* xy, const int32_t* pt_poly, const PolyRec* polys, const PolyAnn* anns,
                             const long long* edge_start, const PolyBig* big, const PolyBig* h_big, int n_big, unsigned long long* keys, int32_t* cov,
                             uint32_t* bnd, uint32_t* nb, uint32_t* nruns, uint32_t* areas, int32_t* bboxes);
// run_offsets = the exclusive prefix of nruns (n + 1 entries)
void poly_offsets_forward(hipStream_t s, const uint32_t* nruns, long n, long long* run_offsets);
// counts[run_offsets[k] ..] = the differences of annotation k's boundaries, closed by the run to h*w
void poly_write_forward(hipStream_t s, const PolyAnn* anns, long n_anns, const long long* tog_off, const uint32_t* bnd, const uint32_t* nb,
                        const long long* run_offsets, uint32_t* counts);

// ================================================================================================
// Run-length masks -> polygon rings (mrcnn_rle_to_polygons; kernels_polygons.hip, the rule is polygon_rule.h).  All tables are device
// arrays.  A UNIT is one vertex column X (0..w) of one RLE; its corners come from merging the runs of pixel columns X-1 and X.  The
// corners of the whole set lie back to back in unit order — per RLE by (X, Y): the order that names a ring's start — and a corner is
// polygon_rule.h's 32-bit word.  Every corner has one successor in the walk; the rings are the cycles of that permutation.
// ================================================================================================
constexpr int POLYGON_LDS_CORNERS = MRCNN_POLYGON_LDS_CORNERS;   // corners an RLE may have to be sorted and ranked by one block in LDS (24 KiB)
struct PolygonImage { long long unit0; int h, w; };              // image b: its first unit (slots * (w + 1) units follow) and its sides
struct PolygonSet {
    const uint32_t* pre_b;            // rle_prefix_forward's B, indexed like counts
    const long long* run_offsets;
    const unsigned long long* totals; // rle_prefix_forward's totals: an RLE that does not sum to its plane is not walked
    const PolygonImage* tab;
    int n_images, slots;
    long long units;
    uint32_t* unit_cnt;               // units: the corners of a unit (always even)
    unsigned long long* unit_start;   // units + 1: their exclusive prefix
    long long* corner0;               // n + 1: the first corner of RLE k
};
// unit_cnt, unit_start and corner0, and summary[0..2] = the lowest k whose total is not its plane's h*w (~0: none), the corners of the
// set, the most corners of one RLE.  The caller reads the summary back before it sizes and launches anything else.
void polygons_count_forward(hipStream_t s, const PolygonSet& set, unsigned long long* summary);
struct PolygonWork {                  // n_corners entries each unless said otherwise
    uint32_t* corner;                 // polygon_rule.h's word
    uint32_t *succ, *lead, *dist;     // the next corner of the walk, the smallest corner of its ring, the steps from here to that one
    uint32_t *head, *len;             // 1 / the ring's length at a ring's smallest corner, else 0
    unsigned long long *ring_id, *vertex0;   // n_corners + 1: the exclusive prefixes of head and len
    // RLEs above POLYGON_LDS_CORNERS only: slices padded to a power of two (sort, the sum of the padded sizes <= 2 * n_corners), the
    // padded sizes and their prefix (n, n + 1), and the two sides of the pointer jumping
    unsigned long long* sort; uint32_t* pad_size; unsigned long long* pad_start;
    uint32_t *next_a, *next_b; unsigned long long *md_a, *md_b;
};
// The walk's permutation, every ring's leader and every corner's rank, then rle_rings (n + 1, device).  n_corners and most (the summary's)
// size the launches: with R = ceil(log2(most)), R * (R + 3) / 2 + 5 more when most > POLYGON_LDS_CORNERS; never the number of RLEs.
void polygons_trace_forward(hipStream_t s, const PolygonSet& set, const PolygonWork& w, long long n_corners, long long most, long long* rle_rings);
// ring_offsets (n_rings + 1), ring_areas (n_rings, may be nullptr) and xy (2 * n_corners), every vertex at its final place
void polygons_write_forward(hipStream_t s, const PolygonWork& w, long long n_corners, long long n_rings, long long* ring_offsets, long long* ring_areas,
                            int32_t* xy);

// ================================================================================================
// Polygon rings simplified (mrcnn_polygons_simplify; kernels_simplify.hip, the rule is simplify_rule.h).  All tables are device arrays.
// One workgroup owns a ring and runs its chains level by level: in LDS for a ring of at most SIMPLIFY_LDS_VERTICES vertices, in its own
// carve of the global scratch above.  Three launches and one scan, whatever the number of rings and the depth of the recursion.
// ================================================================================================
constexpr int SIMPLIFY_LDS_VERTICES = MRCNN_SIMPLIFY_LDS_VERTICES;
struct SimplifyRings { const long long* ring_offsets; const int32_t* xy; long long n_rings; };
// summary[0..3] = the lowest ring whose offsets are negative, decrease or span 2^31 vertices (~0: none), the lowest ring with a
// coordinate outside 0..32767 (~0: none; not looked for when summary[0] names a ring), the most vertices of one ring, ring_offsets[n_rings].
void simplify_check_forward(hipStream_t s, const SimplifyRings& in, unsigned long long* summary);
struct SimplifyWork {
    uint8_t* keep;                    // per input vertex: it stays
    uint32_t* count;                  // n_rings: the vertices a ring keeps
    // rings above SIMPLIFY_LDS_VERTICES only, per input vertex (nullptr when there is none): the chain a vertex is in, and the two sides of the slots
    unsigned long long *chain, *slot_a, *slot_b;
};
// keep and count by the rule, then out_ring_offsets (n_rings + 1) = the exclusive prefix of count; its last entry is the size needed
void simplify_count_forward(hipStream_t s, const SimplifyRings& in, unsigned long long E, const SimplifyWork& w, long long* out_ring_offsets);
// the kept vertices at their places: out_xy, out_src_index (may be nullptr) and out_areas2 (may be nullptr); n_out = out_ring_offsets[n_rings]
void simplify_write_forward(hipStream_t s, const SimplifyRings& in, const SimplifyWork& w, const long long* out_ring_offsets, long long n_out,
                            long long* out_areas2, int32_t* out_xy, long long* out_src_index);

// ================================================================================================
// Polygon rings nested into outlines and their holes (mrcnn_polygons_nest; kernels_nest.hip, the rule is nest_rule.h).  All tables are
// device arrays.  One workgroup owns a target ring and its waves the candidates of the ring's RLE; eight launches and two scans, whatever
// the number of rings and RLEs.
// ================================================================================================
struct NestRings { const long long* rle_rings; long long n_rles; const long long* ring_offsets; const int32_t* xy; long long n_rings; };
struct NestWork {
    unsigned long long* size;         // n_rings: |area2|
    int4* box;                        // n_rings: the smallest and the largest x and y of a ring's vertices (x, y, z, w); an empty ring holds nothing
    int32_t* rle;                     // n_rings: the RLE that owns the ring
    uint32_t *shell, *holes, *rings;  // n_rings each: the depth is even; a shell's holes; a shell's polygon's rings (0 for a hole)
    unsigned long long *polygon, *start;      // n_rings + 1 each: the shells before a ring; the rings of the polygons before a ring
};
// summary[0..2] = the lowest RLE at which rle_rings does not start at 0, decreases or does not end at n_rings, the lowest ring whose
// offsets are negative, decrease or span 2^31 vertices, the lowest ring with a coordinate outside 0..32767 (~0: none; the last is not
// looked for, and size, box and rle are not written, when one of the first two names something).
void nest_measure_forward(hipStream_t s, const NestRings& in, const NestWork& w, unsigned long long* summary);
// the five arrays of the entry from rings that passed; polygon[n_rings] is then the number of polygons
void nest_forward(hipStream_t s, const NestRings& in, const NestWork& w, long long* parent, int32_t* depth, long long* rle_polys, long long* poly_rings,
                  long long* ring_order);

// ================================================================================================
// Measuring run-length masks (mrcnn_rle_measure, mrcnn_rle_convex_hull; kernels_rle_shape.hip, the rules are shape_rule.h).  All tables
// are device arrays.
// ================================================================================================
// A ring's candidates, segments and slots live in LDS up to this many vertex columns (w + 1 <= HULL_LDS_COLUMNS), in global scratch above.
// Per vertex column two candidate positions (top and bottom chain), each an 8-byte slot, a 4-byte row and a 4-byte segment: 32 bytes, so
// 4096 columns take 128 KiB of the 160 KiB a workgroup can have.
constexpr int HULL_LDS_COLUMNS = MRCNN_HULL_LDS_COLUMNS;
constexpr int HULL_LDS_BYTES_PER_COLUMN = 32;
static_assert((long long)HULL_LDS_COLUMNS * HULL_LDS_BYTES_PER_COLUMN <= 159 * 1024, "MRCNN_HULL_LDS_COLUMNS: a ring's work must fit a workgroup's LDS");
// the set: heights, widths and rle_prefix_forward's totals per RLE, its B per run; vcol0 (n + 1) = the vertex columns (w + 1 per RLE)
// before RLE k, vcols their number
struct ShapeSet {
    const uint32_t* counts; const uint32_t* pre_b; const long long* run_offsets;
    const int32_t* heights; const int32_t* widths; const unsigned long long* totals; const long long* vcol0;
    int n; long long vcols;
};
// *bad (device, one word) = the lowest k whose total is not its plane's h*w, ~0 if all are right: the caller reads it back first
void rle_shape_check_forward(hipStream_t s, const ShapeSet& S, unsigned long long* bad);
// measures (n x 7): one fill and two launches
void rle_shape_measure_forward(hipStream_t s, const ShapeSet& S, long long* measures);
struct HullWork {
    int2* ext;                        // vcols: (t, b) of a pixel column, (-1, -1) for an empty one and for the entry of vertex column w
    uint8_t* keep;                    // 2 * vcols: per candidate position, it is a hull vertex
    uint32_t* count;                  // n: the vertices of a hull
    // RLEs wider than HULL_LDS_COLUMNS - 1 only, per candidate position (nullptr when there is none): the segment a candidate is in, the slots
    uint32_t* chain; unsigned long long* slot;
};
// ext, keep and count by the rule, then hull_offsets (n + 1) = the exclusive prefix of count; max_w = the widest RLE.  Three launches.
void rle_hull_count_forward(hipStream_t s, const ShapeSet& S, const HullWork& W, int max_w, long long* hull_offsets);
// the rings at their places: xy (n_out = hull_offsets[n] vertices), areas2 and obb (either may be nullptr).  Two launches.
void rle_hull_write_forward(hipStream_t s, const ShapeSet& S, const HullWork& W, const long long* hull_offsets, long long n_out, int32_t* xy,
                            long long* areas2, long long* obb);

// COCOeval.accumulate (mrcnn_coco_accumulate; kernels_coco_acc.hip).  -ffp-contract=off.  All tables are device arrays.
// A chunk is COCO_ACC_CHUNK consecutive entries of one category's segment [seg0, seg0 + seg_len) of the flat detection list, starting
// `at` entries into it (a multiple of the chunk); the chunks of all segments, in order, are the grid of the sort kernels.
constexpr int COCO_ACC_CHUNK = MRCNN_COCO_ACC_CHUNK;
struct AccChunk { long long seg0; int seg_len, at; };
// Stable sort of every segment by descending score (-0 = 0, NaN last).  `longest` = the longest segment.  keys / perm a and b hold n_dt
// entries each; returns the one of perm_a / perm_b that holds the result: perm[i] = the entry that stands at sorted position i.
// 1 + ceil(log2(longest / COCO_ACC_CHUNK)) launches.
const uint32_t* coco_acc_sort_forward(hipStream_t s, const double* scores, const AccChunk* chunks, long n_chunks, long long longest,
                                      unsigned long long* keys_a, uint32_t* perm_a, unsigned long long* keys_b, uint32_t* perm_b);
// code[pl * n_dt + i] = 2 if ignore else matched, of the entry at sorted position i, for each of the `planes` = A * T planes; srank[i] = its rank
void coco_acc_permute_forward(hipStream_t s, const uint32_t* perm, const int32_t* ranks, const uint8_t* matched, const uint8_t* ignore, long long n_dt,
                              int planes, uint8_t* code, int32_t* srank);
// precision (T, R, K, A, M) and recall (T, K, A, M), every entry written; one block per (k, a, m, t)
void coco_acc_scan_forward(hipStream_t s, const uint8_t* code, const int32_t* srank, const long long* cat_off, const long long* npig,
                           const int32_t* max_dets, const double* rec_thrs, long long n_dt, int K, int A, int M, int T, int R, double* precision,
                           double* recall);

}  // namespace mrcnn
