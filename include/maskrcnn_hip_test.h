/*
 * maskrcnn_hip_test.h — TEST AND MEASUREMENT entry points of libmaskrcnn_hip.so.
 *
 * Not part of the drop-in surface (include/maskrcnn_hip.h): these are what tests/, tools/ and bench.py use to run one
 * convolution of the kernel family on caller data, to time a layer shape, to read the live per-kernel profile of a
 * predict, and to switch kernel-selection policy for A/B comparisons.  The switches are PROCESS-WIDE and not
 * thread-safe; a production host never calls anything declared here.
 *
 * mrcnn_test_proposals_batch / mrcnn_test_detections_batch run the box path (top-k select, sort and decode, suppression matrix, greedy scan,
 * final top-k) on a batch of caller images in one launch sequence with a predict's bindings and strides: the tests' way to put adversarial
 * content — empty and saturated neighbours, tied scores, odd anchor counts, more than 1024 regions, class ids beyond 1024 — where only
 * whole-model predicts on random weights reached before.  mrcnn_test_mask_select_batch does the same for the mask head's row selection: rows
 * dropped in the middle of an image, where compact index and row differ, in each of the three tail forms.
 */
#ifndef MASKRCNN_HIP_TEST_H
#define MASKRCNN_HIP_TEST_H

#include "maskrcnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Live per-kernel profile of the convolution family during predict (bench.py roofline leg): when
 * enabled every conv launch is bracketed by HIP events on the model's stream.  tile: 0 = the
 * 128x128 kernel, 1 = 128x64, 2 = 128x32, 3 = 128x128 run by four waves of 32x128 (split modes, K >= 2048), 4 = 256x256 ping-pong,
 * 5 = the persistent halo tiles of the 3x3 layers of the split modes (kernels_conv_halo.hip), 6 = halo tiles with the fused
 * bottleneck tail (a 3x3 `branch2b` and the 1x1 `branch2c` behind it in one launch; flops of both layers).  enable(1) opens a measurement window (totals reset);
 * enable(0) closes it and the totals stay readable — the events cost ~2 % (fp32) / ~13 % (fp16) of a step,
 * so bench.py opens the window for the first steps of its timed region only.
 * total_flops is ALGORITHMIC work (2*M*N*K of the convolution, padding excluded). */
MRCNN_API int mrcnn_model_conv_profile_enable(mrcnn_model* model, int on);
MRCNN_API int mrcnn_model_conv_profile_get(mrcnn_model* model, int tile, int64_t* launches, double* total_ms,
                                           double* total_flops);
/* The same window split in two groups: 1 = the BACKBONE convolutions (conv1 and the res2..res5 stages: SURVEY.md section 8d's 344.9 GFLOP per image,
 * the subset north_star's ">= 50 % MFMA roofline" is worded on), 0 = every other convolution (FPN, RPN, heads). */
MRCNN_API int mrcnn_model_conv_profile_group(mrcnn_model* model, int group, int64_t* launches, double* total_ms, double* total_flops);
/* The same totals broken down by GEMM shape (M = images*OH*OW, N = output columns, K = taps*Cin): writes at
 * most `capacity` records, *count = number of distinct shapes seen (call with capacity 0 to size the buffer). */
typedef struct mrcnn_conv_shape_stat {
    int32_t M, N, K, tile;
    int64_t launches;
    double total_ms, total_flops;
    double total_bytes;      /* ALGORITHMIC bytes: every operand of the layer across HBM once (inputs read, filters, residual, outputs stored) */
} mrcnn_conv_shape_stat;
/* ALGORITHMIC bytes of the launches counted in tile class `tile` (as mrcnn_model_conv_profile_get's totals): what a memory-bound class is priced
 * against (bench.py: roofline.by_tile_class[*].bound / frac_of_hbm). */
MRCNN_API int mrcnn_model_conv_profile_bytes(mrcnn_model* model, int tile, double* total_bytes);
MRCNN_API int mrcnn_model_conv_profile_shapes(mrcnn_model* model, mrcnn_conv_shape_stat* out, int capacity, int* count);

/* ---------------------------------------------------------------------------------------------
 * Convolution micro-benchmark hook (bench.py roofline leg): runs one convolution of the trunk's
 * kernel family on synthetic data resident in HBM and reports the average kernel time measured
 * with HIP events on the launching stream.
 * --------------------------------------------------------------------------------------------- */
MRCNN_API int mrcnn_bench_conv(int batch, int h, int w, int cin, int cout, int ksize, int stride,
                               int iters, float* avg_ms, double* flops);
/* Same with an explicit element type (MRCNN_F32 | MRCNN_F16, fp32 accumulate). */
MRCNN_API int mrcnn_bench_conv_dtype(int batch, int h, int w, int cin, int cout, int ksize, int stride,
                                     int iters, int dtype, float* avg_ms, double* flops);

/* What the matrix cores of THIS board sustain right now: every wave of the chip on back-to-back MFMAs (kind MRCNN_F16: v_mfma_f32_32x32x16_f16,
 * MRCNN_F32: v_mfma_f32_32x32x2_f32) whose register operands change from one instruction to the next, no operand traffic, for `seconds`
 * (<= 30); *tflops = the rate over the last third of the run, *mhz_equivalent (optional) = the shader clock it means at back-to-back issue.
 * bench.py runs it in-process before the timed loop (`roofline.sustained_peak_live`): boxes of one pool differ by several per cent under
 * the power cap, and this is what separates a kernel change from a box change. */
MRCNN_API int mrcnn_bench_mfma_probe(double seconds, int kind, double* tflops, double* mhz_equivalent);

/* One convolution of the engine's kernel family on caller (host) data — the unit the parity tests of the kernels use:
 * in (B,H,W,Cin) NHWC fp32, filters (Cout, k, k, Cin) fp32 (k = 1 | 3, 'same' padding k/2), optional per-channel
 * scale/shift (folded BatchNorm + bias), optional residual (B,OH,OW,Cout), act 0 none | 1 ReLU | 2 sigmoid;
 * dtype = compute mode (inputs are converted to it on the host, round-to-nearest); out (B,OH,OW,Cout) fp32
 * (MRCNN_F16: the fp16 values the layer stores, widened).  mrcnn_debug_set switches kernel-selection policy knobs for A/B tests
 * ("conv_pp" 0|1: the 256-row ping-pong fp16 kernels; "conv_pp_min_tiles", "conv_pp_min_kt", "conv_pp_min_fill", "conv_pp_split",
 * "conv_pp_dbg"; "conv_tn4" -1|0|1: split modes, 128x128 tile as 4 waves of 32x128 by policy | never | always; "conv_min_blocks": the grid
 * size below which the N tile is narrowed; "conv_direct" 0|1|2|3: epilogue without block barriers never | fp16 tensors straight from the accumulators | + fp32 tensors through wave-private LDS tiles | + the fp16 tensors of the 128-column kernel (default 3; all four bit-identical); "mask_fused" 0|1: the mask head's
 * deconvolution + selected-class 1x1 as two launches over a materialised tensor | fused — results within fp32 summation noise): every choice must give
 * bit-identical results — the tile shape depends on the batch size and per-image results must not.  Further knobs: "conv_halo" 0|1 the
 * persistent halo kernel of the 3x3 layers of the split modes (its K order is its own: results differ from "0" by summation noise);
 * "halo_geo" 0|1: its round-3 tile geometries | two-row tiles, region-sized staging, conflict-free LDS pitch (bit-identical);
 * "conv_tail" 0|1: bottleneck tails as two launches | one fused launch where the grid fills the chip (bit-identical; default 0: measured slower);
 * "conv_stem" 0|1|2: conv1 and the max-pool as two launches | one fused launch (default; split modes: bit-identical to 0) | fp16 tensors: the fused launch in
 * round 4's four-K-group form (bit-identical to 0; the default compact form — two K groups per kernel row, half the MFMAs — differs from it by summation noise);
 * "halo_lat" 0|1|2: 3x3 layers on grids under 3/8 of the chip (single images at C5 / P5): the eight-wave 64 x 128 tiles | 64 x 64 tiles on
 * four waves with deep prefetch (default) | that form for every grid under 3/4 (bit-identical);
 * "halo_n64" 0|1|2: 64-column 3x3 layers of the split modes on the 64-column 128-row kernel | on the halo kernel as 128 x 64 tiles | and as 256 x 64 tiles where
 * four image rows x 64 columns tile the level and the grid fills the chip (default 2; 1 and 2 are bit-identical, "0" differs by summation noise: its K order is
 * the 128-row kernel's);
 * "halo_rounds" 0|1: 128 x 128 halo tiles whenever the grid covers 3/4 of the chip | 64 x 128 where they shorten a nearly empty last round (default 1; bit-identical);
 * "mask_sel_wave" 0|1: the mask head's deconvolution + selected-class dot through the block-staged epilogue (128-column partial sums) | straight from the
 * accumulators (64-column partial sums; default 1) — the two differ by summation noise;
 * "conv_scfuse" 0|1: a ResNet stage's shortcut convolution as its own launch | inside the launch of the `branch2c` that adds it (default 1; bit-identical);
 * "conv_kchunk" 0|1: the long-K (>= 2048) 1x1 layers of the split modes as one running sum | as 4 / 8 canonical K chunks folded in order
 * (default 1; the two differ by summation noise — the chunk count is a property of the layer, never of the batch);
 * "conv_ksplit" 0|1 and "conv_ksplit_below" n: chunked layers whose widest-tile grid has fewer than n (256) blocks give every chunk its
 * own block, the last one to finish folds the partial sums | never (bit-identical to each other).
 * "conv_min_blocks_split" n: the same threshold for the split modes alone (default 256 = one block per CU; fp16 tensors keep 448; bit-identical);
 * box path (kernels_boxes.hip; none changes an output bit): "proposal_rank_sort" 0|1: the K pre-NMS candidates ordered by one bitonic-sort block per
 * image | by rank counting over the whole chip (default 1); "nms_col_splits" n: column splits of the suppression-matrix grid (0 = by policy: as many
 * as the chip's wave slots hold, at least 4); "nms_class_fast" 0|1: DetectionLayer's per-class limit tested per chunk as count + 64 | as count + the
 * chunk's own alive candidates of the class, classes at the limit dropping out (default 1).
 * Measurement-only environment variable read by mrcnn_model_load: MRCNN_CU_MASK_PROBE="w0,...,w7" (hexadecimal) creates the handle's stream on that subset of the
 * CUs (hipExtStreamCreateWithCUMask) — tools/dual_stream_probe.py's question whether two half batches on disjoint halves of the chip beat one batch on all of it (no).
 * The switches are PROCESS-WIDE test / measurement knobs: not thread-safe; a choice captured in a hipGraph stays captured.
 * ARMING (round 6): mrcnn_debug_set, the MRCNN_* environment overrides of the switches' defaults and the measurement hooks (MRCNN_CU_MASK_PROBE,
 * MRCNN_BNECK_DBG, MRCNN_SPLIT_EXP, MRCNN_BENCH_RESIDUAL) work only in a process started with MRCNN_TEST_KNOBS=1 in its environment (tests/conftest.py
 * and the tools set it; read once, at the library's first use).  Anywhere else — every production host — mrcnn_debug_set returns MRCNN_ERR_UNSUPPORTED
 * and the overrides are ignored: the alternative forms stay in the library as the tests' bit-identity anchors, out of a host's reach
 * (tests/test_host.py::test_the_knobs_are_out_of_a_production_hosts_reach).  Forms that lost their A/B and anchor nothing are removed instead
 * (round 6: the level-parallel FPN / RPN region of round 5). */
MRCNN_API int mrcnn_conv2d_nhwc(const float* in, int batch, int h, int w, int cin, const float* filters, int cout,
                                int ksize, int stride, const float* scale, const float* shift, const float* residual,
                                int act, int dtype, float* out);
MRCNN_API int mrcnn_debug_set(const char* key, int value);

/* An identity ResNet bottleneck block of the fp16 mode on caller (host) data: x (B,H,W,4C) fp32 (rounded to fp16 on the host),
 * w1 (C,4C), w2 (C,3,3,C), w3 (4C,C) fp32 (rounded to fp16), folded BatchNorm scale / shift per layer; out (B,H,W,4C) = the fp16
 * values the block stores, widened.  fused = 1: ONE persistent launch with both mid tensors on chip (kernels_bneck.hip; needs
 * C in {64,128,256}, W % 16 == 0, H % 16 == 0 (C = 256: H % 8 == 0)); fused = 2: the same with every operand staged through LDS (C = 256
 * otherwise streams its filter fragments straight into registers); fused = 0: the three launches of the convolution family.
 * All must agree bit for bit (tests/test_gpu_bneck.py).  iters > 0: *avg_ms = average time of `iters` further runs (HIP events).
 * "conv_bneck" 0|1|2|3 of mrcnn_debug_set: the engine's identity bottlenecks of the fp16 mode as three launches | fused where the grid
 * fills the chip (default) | fused, all-LDS form | fused at every grid size (bit-identical, all four). */
MRCNN_API int mrcnn_bottleneck_nhwc(const float* x, int batch, int h, int w, int cmid, const float* w1, const float* w2, const float* w3,
                                    const float* s1, const float* h1, const float* s2, const float* h2, const float* s3, const float* h3,
                                    int fused, int iters, float* out, float* avg_ms);
/* The stage-ENTRY block of C2 (res2a; fp16 mode): x (B,H,W,C) with C = 64, w1 (C,C), w2 (C,3,3,C), w3 (4C,C), ws (4C,C) = the shortcut convolution
 * `branch1`; bn[8] = scale / shift of branch2a, 2b, 2c, branch1 in that order; out (B,H,W,4C).  fused = 1: one launch, 0: the four launches — bit for bit. */
MRCNN_API int mrcnn_bottleneck_first_nhwc(const float* x, int batch, int h, int w, int cmid, const float* w1, const float* w2, const float* w3, const float* ws,
                                          const float* const bn[8], int fused, int iters, float* out, float* avg_ms);

/* A chained pair of the split modes on caller (host) data (dtype MRCNN_F32S | MRCNN_F32X3): P = a bottleneck's `branch2c`, t2 (B,H,W,C) x w3 (4C,C) with
 * folded BatchNorm s3 / h3, plus EITHER the residual x (B,H,W,4C) OR (x == NULL) the shortcut convolution ws (4C,cs) with s_s / h_s over xs
 * (B, H*ss, W*ss, cs) sampled with stride ss, then ReLU -> y (B,H,W,4C); Q = the next block's `branch2a`, y x w1 (C,4C) with s1 / h1, ReLU -> t1 (B,H,W,C).
 * chained = 1: ONE launch (kernels_conv_chain.hip; needs C in {64,128,256}) at whatever grid size; 0: the two launches of the convolution family.
 * C = 256 runs the identity form only (the residual x): with the shortcut's operands and chained = 1 it fails with MRCNN_ERR_UNSUPPORTED.
 * in_place = 1: y is written over the residual (the engine's form).  Both outputs must agree bit for bit (tests/test_gpu_conv_chain.py,
 * tests/test_gpu_conv_chain_c256.py); the watchdog word of the call: mrcnn_test_last_range_flag.
 * "conv_chain" 0|1|2 of mrcnn_debug_set: the engine's C2 / C3 pairs as two launches | C2's pairs chained where the grid fills the chip (default; C3's measured
 * slower and stay two launches) | every pair chained at every grid size (bit-identical, all three).
 * "conv_chain4" 0|1|2: the same for C4's identity pairs (C = 256), a knob of their own. */
MRCNN_API int mrcnn_conv_chain_nhwc(const float* t2, int batch, int h, int w, int cmid, const float* w3, const float* s3, const float* h3, const float* x,
                                    const float* xs, int cs, int ss, const float* ws, const float* s_s, const float* h_s,
                                    const float* w1, const float* s1, const float* h1, int dtype, int chained, int in_place, float* y, float* t1);

/* The stream image of one filter of a chainable C = 256 pair, as the engine packs it when a model is loaded (csrc/conv_pack.h; needs no GPU):
 * w (4*cmid, cmid) with q = 0 (P, `branch2c`) or (cmid, 4*cmid) with q = 1 (Q, `branch2a`), cmid = 256; image: 4*cmid*cmid fp16 values. */
MRCNN_API int mrcnn_test_chain_stream_image(const float* w, int cmid, int q, uint16_t* image);

/* The consecutive identity blocks of a C = 256 stage (C4's 22 in ResNet-101) on caller data: x (B,H,W,1024), stacked operands w1 (n,256,1024),
 * w2 (n,256,3,3,256), w3 (n,1024,256), bn = {s1,h1,s2,h2: (n,256); s3,h3: (n,1024)}.  form 1: ONE launch in which a tile's block l waits for its
 * neighbour tiles' block l - 1 (kernels_bneck.hip, STAGE form); form 0: one fused launch per block.  Bit-identical (tests/test_gpu_bneck.py).
 * out (B,H,W,1024) = the last block's output; *status_flag (optional) = the launch's flag word (bit 0 fp16 range, bit 1 "no progress").
 * "conv_bneck_stage" 0|1 of mrcnn_debug_set: the engine's C4 identity blocks of the fp16 mode one launch per block (default) | one launch per stage
 * (measured equal: profiles/r06_bneck_stage_ab.txt). */
MRCNN_API int mrcnn_bottleneck_stage_nhwc(const float* x, int batch, int h, int w, int nlayers, const float* w1, const float* w2, const float* w3,
                                          const float* const bn[6], int form, int iters, float* out, float* avg_ms, int* status_flag);

/* The fp16-range watchdog word of the calling thread's last mrcnn_conv2d_nhwc / mrcnn_test_conv_form_nhwc / mrcnn_conv_chain_nhwc / mrcnn_bottleneck_nhwc / mrcnn_bottleneck_first_nhwc (each of them
 * gives its launches a zeroed 4-byte device flag, the way the engine does for a predict, and reads it back when they have finished):
 * bit 0: some stored output has !(|v| < 65504) after scale, shift, residual and activation (NaN included) — what makes MRCNN_F16 refuse a predict and
 * MRCNN_F32S / MRCNN_F32X3 recompute it.  Padded columns, rows beyond M, the on-chip lanes of no real output and, in the selected-class mode
 * (where the watched value is the activated y the dot reads), ROI rows of class -1 never set it; in the fused bottlenecks
 * the two mid tensors count as stored outputs.  MRCNN_F32 (exact fp32: no fp16 hand-over) leaves the word 0; so does an entry that failed.
 * mrcnn_bottleneck_stage_nhwc returns its word through status_flag.  tests/test_gpu_range_watch.py pins every epilogue form with it. */
MRCNN_API int mrcnn_test_last_range_flag(int* flag);

/* ONE conv_forward of a form only the engine builds, on caller (host) data, in any of the four compute modes — what mrcnn_conv2d_nhwc's dense
 * description cannot reach (tests/test_gpu_conv_forms.py; the float64 definitions: tests/conv_forms_cases.py).  The layer reads a level of
 * batch x h x w pixels of cin channels and has cout output channels; ksize 1 | 3 ('same' padding ksize/2), stride, act 0 | 1 | 2 as mrcnn_conv2d_nhwc.
 *   in        dense (batch, h*in_step, w*in_step, cin); in_step 1 | 2: the layer reads every in_step-th row and column through its strides
 *             (the RPN's shared layer on P6 reads P5 this way).
 *   filters   (cout, ksize, ksize, cin); deconv2 = 1: (2, 2, cout, cin) = (dy, dx, co, ci) of the transposed 2x2 stride-2 convolution
 *             (ksize 1, stride 1, in_step 1), packed by the engine's own routine (csrc/conv_pack.h).  scale / shift: cout entries or NULL (1 / 0).
 *   residual  NULL or (batch, OH, OW, cout); res_shift = 1: (batch, ceil(OH/2), ceil(OW/2), cout), read at (oh >> 1, ow >> 1) — the FPN laterals.
 *   outputs   n_split = 0: every column goes to `out`; n_split > 0: columns [0, n_split) go to `out`, the rest to `out2` (the unfused RPN heads).
 *             Output k is a buffer of len elements; image b starts at element offset + b * batch_stride, its pixel p at p * pitch (pitch >= the
 *             output's columns; 0 = dense).  deconv2: the output image is 2h x 2w, pixel (y, x) at y * row_pitch + x * pitch (row_pitch 0 = 2w * pitch).
 *             Each buffer is filled with `sentinel` before the launch and returned WHOLE in out / out2 (fp32; fp16 stores widened: pass a
 *             sentinel fp16 holds), so a caller sees every element the launch did not address.  out_f32 = 1 (MRCNN_F16 only): fp32 stores.
 *   sel_w     non-NULL with deconv2: the selected-class dot instead of the store (ConvDesc::sel_partial) — sel_w (nc, cout), sel_cid (batch) with
 *             values < 0 = "row not written".  sel_partial receives batch * 4*h*w * parts floats, sentinel-filled first, *sel_parts = parts =
 *             cout / (64 | 128 by "mask_sel_wave"); a caller sizes it for cout / 64.  Nothing goes to `out` (may be NULL).
 * dtype = the compute mode; operands are converted on the host as in mrcnn_conv2d_nhwc, padded filter rows are zero and carry a shift far
 * beyond the fp16 range.  The watchdog word of the call: mrcnn_test_last_range_flag.  A combination the dispatcher cannot run fails with a
 * message (MRCNN_ERR_INVALID / _SHAPE / _UNSUPPORTED); nothing falls back. */
typedef struct mrcnn_test_conv_output {
    float* data;                   /* len floats, host */
    int64_t len, offset, batch_stride, pitch, row_pitch;
} mrcnn_test_conv_output;
typedef struct mrcnn_test_conv_form {
    int32_t dtype, batch, h, w, cin, cout;
    int32_t ksize, stride, act, in_step, res_shift, n_split, deconv2, out_f32;
    int32_t nc, reserved;
    float sentinel;
    int32_t reserved2;
    const float* in;
    const float* filters;
    const float* scale;
    const float* shift;
    const float* residual;
    const float* sel_w;
    const int32_t* sel_cid;
    mrcnn_test_conv_output out, out2;
    float* sel_partial;
    int32_t* sel_parts;
} mrcnn_test_conv_form;
MRCNN_API int mrcnn_test_conv_form_nhwc(const mrcnn_test_conv_form* form);

/* The classifier head behind its last inner product, on caller (host) rows: logits (n rows at stride ld >= nc, the first nc entries of a row are read),
 * bbox (n, nc*4) -> probs_out (n, nc) = the row softmax, cls6_out (n, 6) = (dy, dx, dh, dw, class id, score) of the arg-max class (ties -> lowest index).
 * NaN entries never win; a row with no comparable entry (all probabilities NaN: one logit +Inf or NaN, or all -Inf) yields class 0, its score the
 * row's probability at index 0 (the NaN as it is) and class 0's deltas: DetectionLayer drops such a row (score >= threshold is false). */
MRCNN_API int mrcnn_classifier_rows(const float* logits, int64_t ld, const float* bbox, int nc, int64_t n, float* probs_out, float* cls6_out);

/* The NHWC ROIAlign sampler as the fused engine launches it — a BATCH of images in one launch, every pyramid level with its own power-of-two
 * multiplier — on caller (host) data; mrcnn_roi_align_nhwc reaches neither (one image, multipliers 1).  maps[l] (batch, H_l, W_l, channels) fp32,
 * converted on the host to `dtype` (MRCNN_F32 | MRCNN_F16, round-to-nearest: pass fp16-representable values for MRCNN_F16); level_mul[l]: every
 * sample of level l is multiplied by it in fp32 before the predicate and the store; rois (batch, n_rois, roi_stride) rows (y1,x1,y2,x2,...);
 * out (batch, n_rois, pool, pool, channels) fp32 (MRCNN_F16: the fp16 values the kernel stores, widened); row_flags (optional, batch x n_rois
 * int32): 1 iff every fp32 sample times multiplier of the row != 0.  channels % 4 == 0, roi_stride >= 4, n_rois >= 1, batch >= 1
 * (tests/test_gpu_roi_align_nhwc.py). */
MRCNN_API int mrcnn_test_roi_align_nhwc_batch(const float* const maps[4], const int heights[4], const int widths[4], int channels, int dtype,
                                              const float level_mul[4], const float* rois, int64_t roi_stride, int n_rois, int batch, int pool,
                                              double image_w, double image_h, float* out, int32_t* row_flags);

/* The proposal path and the detection path (csrc/kernels_boxes.hip) on a BATCH of caller (host) images in one launch sequence, bound and strided
 * exactly as a predict does it — the layer API (mrcnn_layer_evaluate) binds one image with every batch stride 0 and so never reaches the
 * per-image state / histogram / count words, the image index of the grids or the batch-dependent column-split policy (tests/test_gpu_boxes.py;
 * the cases and their conditions: tests/boxes_cases.py).
 *   mrcnn_test_proposals_batch: probs (batch, n_anchors, 2), deltas (batch, n_anchors, 4), anchors (n_anchors, 4) passed in (no anchors file),
 *     std4 = bboxStdDev; K = min(n_anchors, pre_nms) candidates, batch strides 2A / 4A.  rois (batch, max_proposals, row_stride >= 4) is IN/OUT:
 *     the caller's buffer is staged to the device first, as the layer does, so columns >= 4 of kept rows come back as they went in and padded
 *     rows come back zero.  keep_count (optional, batch int32): proposals kept per image.
 *   mrcnn_test_detections_batch: rois (batch, n, 4), cls6 (batch, n, 6) = (dy, dx, dh, dw, class id, score); out (batch, max_det,
 *     row_stride >= 6) is IN/OUT in the same way.  n <= 8192 (the greedy scan's LDS); more fails with MRCNN_ERR_UNSUPPORTED and out untouched.
 * Bad arguments return a status; nothing falls back to per-image launches.  The box-path knobs of mrcnn_debug_set apply. */
MRCNN_API int mrcnn_test_proposals_batch(const float* probs, const float* deltas, const float* anchors, int batch, int n_anchors, const float std4[4],
                                         int pre_nms, int max_proposals, float nms_thr, float* rois, int64_t row_stride, int32_t* keep_count);
MRCNN_API int mrcnn_test_detections_batch(const float* rois, const float* cls6, int batch, int n, const float std4[4], int max_det, float score_thr,
                                          float nms_thr, float* out, int64_t row_stride);

/* The mask head's row selection (TimeDistributedMaskLayer.swift:58-89 behind MultiArrayBatchProvider(removeZeros: true); csrc/kernels_elementwise.hip)
 * on a BATCH of caller (host) images in one launch sequence, bound and strided as a predict binds it — the layer API runs one image with every batch
 * stride 0, and the suite's predicts on random weights keep a prefix of the rows, where compact index and row coincide, but for one dropped row in
 * one image, behind the engine's memset (tests/test_gpu_mask_select.py; the cases
 * and the rule's plain restatement: tests/mask_select_cases.py).  The predicate of the first d rows of every image comes from
 *   flags     (batch, d) int32, non-zero = kept: what the engine does (the ROIAlign kernel wrote them; only the compaction runs), OR
 *   pooled    batch images of d rows: row r of image b starts at b * pooled_batch_stride + r * row_stride, its first row_len elements are tested
 *             (row_stride >= row_len, pooled_batch_stride >= d * row_stride; the buffer holds batch * pooled_batch_stride floats), converted on the
 *             host to `dtype` (MRCNN_F32 | MRCNN_F16, round-to-nearest) so that k_mask_row_flags<float | _Float16> runs.  Exactly one of the two.
 * The tail then runs over det_rows >= d rows per image (the layer pads up to the detection count, the engine has det_rows == d):
 *   form 0    mask_select_forward (k_mask_select): feat (batch, d, hw, c) converted to `dtype`, w (nc, c), bias (nc); c % 4 == 0
 *   form 1    mask_select_classes + mask_select_from_partials: partial (batch, d, hw, parts), the layout ConvDesc::sel_partial leaves, bias (nc)
 *   form 2    mask_select_from_full_forward: masks (batch, d, nc, hw)
 *   det       (batch, det_rows, det_stride >= 6): column 4 is the class
 *   out       (batch, det_rows, out_stride >= hw), IN/OUT: the caller's buffer is staged to the device first and returned whole, so a sentinel shows
 *             every element that no launch addressed.  Nothing here zeroes it: the engine's memset in front of the tail stays the engine's.
 *   optional  row_flags (batch, d), mapping (batch, d: only the first kept[b] entries of a row are defined, the rest come back -1), kept (batch),
 *             sel_cid (batch, det_rows: the class table of the fused tail, -1 = row not written; computed in every form when asked for).
 * A null required pointer, both or neither predicate source, form outside 0..2, a dtype other than the two, a count below 1, det_rows < d,
 * parts < 1, a stride below its minimum (MRCNN_ERR_INVALID) or c % 4 != 0 (MRCNN_ERR_SHAPE) fails with a message and leaves `out` untouched;
 * nothing falls back to per-image launches. */
typedef struct mrcnn_test_mask_select {
    int32_t form, dtype, batch, d, det_rows, hw, c, nc, parts, reserved;
    int64_t row_len, row_stride, pooled_batch_stride, det_stride, out_stride;
    const int32_t* flags;
    const float* pooled;
    const float* det;
    const float* feat;
    const float* w;
    const float* bias;
    const float* partial;
    const float* masks;
    float* out;
    int32_t* row_flags;
    int32_t* mapping;
    int32_t* kept;
    int32_t* sel_cid;
} mrcnn_test_mask_select;
MRCNN_API int mrcnn_test_mask_select_batch(const mrcnn_test_mask_select* sel);

/* Measurement (tools/jpeg_ab.py): the wall time of the two stages of the calling thread's last mrcnn_jpeg_decode_batch /
 * mrcnn_maskrcnn_predict_jpegs — host_ms: header parsing + the entropy threads; device_ms: from the upload of the coefficients to the end
 * of the second launch (decode_batch only, where the call waits for it; 0 after predict_jpegs, whose launches run ahead of the predict).
 * With MRCNN_JPEG_ENTROPY_DEVICE host_ms runs from the headers to the verdict words: marker scan, upload of the bytes, the entropy launches, their synchronise
 * and any fallback; device_ms is the inverse DCT and the colour conversion as before. */
MRCNN_API int mrcnn_jpeg_last_stage_ms(float* host_ms, float* device_ms);

/* The quantised coefficients of a batch of JPEG files — what the entropy stage hands to the inverse DCT — from the host decoder
 * (entropy MRCNN_JPEG_ENTROPY_HOST), the device stage (MRCNN_JPEG_ENTROPY_DEVICE) or the sequential host MODEL of the device stage (2:
 * csrc/jpeg_entropy_host.cpp, the same step function phase for phase); HOST and the model need no GPU.  coef (host, `capacity` int16):
 * file b's blocks of 64 (natural order, component after component over the MCU-padded grids) start at block0[b]; block0[batch] = the
 * batch's blocks, written before capacity is checked (too small -> MRCNN_ERR_SHAPE).  Device and model include the fallback: a file they
 * do not call clean is decoded by the host decoder, and a file that one refuses fails the call as "file N of the batch: ...".
 * stats[4] = {files decoded clean on the device / model, files that fell back, most rounds a workgroup needed, units in the batch}.
 * unit_bytes: EVERY per-thread partition of the scan bytes, a power of two in 4..1024 (0 = production, 128); max_rounds: cap of the
 * rounds inside a synchronisation launch and of the launches (0 = production; 1 leaves no round to confirm a state, so every file of
 * more than one unit falls back).  Non-zero knobs work only under MRCNN_TEST_KNOBS=1 (else MRCNN_ERR_UNSUPPORTED); bad values ->
 * MRCNN_ERR_INVALID. */
MRCNN_API int mrcnn_jpeg_coefficients(const mrcnn_jpeg* files, int batch, int entropy, int unit_bytes, int max_rounds, int16_t* coef,
                                      int64_t capacity, int64_t* block0, int32_t* stats);

/* The inverse that mrcnn_rle_transform's device entry works from (csrc/transform_rule.h), evaluated on the host, no GPU: [*lo, *hi) =
 * every integer X with a <= floor((A*X + B) / D) < b, not clipped; empty as *lo >= *hi.  a <= b within +-32768, A, B and D within the
 * limits of a record (else MRCNN_ERR_SHAPE); null lo or hi -> MRCNN_ERR_INVALID.  tests/test_rle_transform_host.py pins the closed form
 * against brute force with it. */
MRCNN_API int mrcnn_test_xf_preimage(int64_t a, int64_t b, int64_t A, int64_t B, int64_t D, int64_t* lo, int64_t* hi);

#ifdef __cplusplus
}
#endif

#endif /* MASKRCNN_HIP_TEST_H */
