/*
 * maskrcnn_hip.h — C ABI of libmaskrcnn_hip.so, the MI355X (gfx950) replacement for the hot path of
 * edouardlp/Mask-RCNN-CoreML.  Plain pointers and sizes only; no C++/torch types.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the reference
 * repo).  All functions return an mrcnn_status (0 = OK) and never abort; the message of the last
 * failure on the calling thread is available from mrcnn_last_error() (the reference throws Swift
 * errors — `extension String: Error`, Sources/Mask-RCNN-CoreML/Utils.swift:13 — or crashes on a
 * force-unwrap, ProposalLayer.swift:68).
 *
 * Threading: handles are not thread-safe; one in-flight call per handle; calls are synchronous
 * (they return after the work on the handle's HIP stream has completed), like Core ML's
 * `evaluate` (ProposalLayer.swift:103).  One model handle per GPU for multi-GPU use.
 *
 * Memory: the caller owns every buffer passed in; the callee never frees them and fully
 * overwrites outputs including zero padding ("CoreML does not erase the memory between
 * evaluations", ProposalLayer.swift:188) — except where the reference itself leaves rows
 * unwritten (TimeDistributedMaskLayer, see below).
 */
#ifndef MASKRCNN_HIP_H
#define MASKRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRCNN_API __attribute__((visibility("default")))

typedef enum {
    MRCNN_OK = 0,
    MRCNN_ERR_INVALID = 1,      /* bad argument / unknown key / wrong dtype                        */
    MRCNN_ERR_IO = 2,           /* file missing or malformed (anchors.bin, *.mrcw)                 */
    MRCNN_ERR_HIP = 3,          /* HIP runtime failure, or no gfx950 device                        */
    MRCNN_ERR_SHAPE = 4,        /* shape / stride mismatch                                          */
    MRCNN_ERR_UNSUPPORTED = 5,
    MRCNN_ERR_CONFIG = 6        /* MaskRCNNConfig URL not set before use                            */
} mrcnn_status;

MRCNN_API const char* mrcnn_last_error(void);
MRCNN_API const char* mrcnn_version(void);
/* Number of visible HIP devices (0 when none; never fails). */
MRCNN_API int mrcnn_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * MLMultiArray mirror (CoreML): 5-D [sequence, batch, channel, height, width], row-major unless
 * strides say otherwise; strides are in ELEMENTS.  The custom layers index with shape[0],
 * strides[0] or strides[2] and the raw data pointer (e.g. ProposalLayer.swift:179,
 * TimeDistributedClassifierLayer.swift:63, PyramidROIAlignLayer.swift:124).
 * --------------------------------------------------------------------------------------------- */
typedef enum {
    MRCNN_F32 = 0, MRCNN_F64 = 1, MRCNN_F16 = 2, MRCNN_U8 = 3, MRCNN_I32 = 4,
    MRCNN_F32S = 5,  /* compute mode only (mrcnn_model_load): fp32 tensors, fp16 filters, split-fp16 MFMA — see there */
    MRCNN_F32X3 = 6, /* compute mode only: as MRCNN_F32S with a three-part split (all 24 significand bits for |a| >= 0.5) */
    MRCNN_DEFAULT = -1 /* compute mode only (mrcnn_model_load): what the ARTEFACT is prepared for — MRCNN_F32X3 when MaskRCNN.mrcw carries
                        * stored split exponents (convert.py --calibrate), MRCNN_F32 otherwise; see mrcnn_model_load */
} mrcnn_dtype;
typedef enum { MRCNN_HOST = 0, MRCNN_DEVICE = 1 } mrcnn_memspace;

typedef struct {
    void*   data;
    int32_t dtype;       /* mrcnn_dtype; the layers assert Float32 inputs (ProposalLayer.swift:108) */
    int32_t memspace;    /* mrcnn_memspace: host buffers are staged over PCIe, device buffers used in place */
    int64_t shape[5];
    int64_t strides[5];  /* elements */
} mrcnn_tensor;

/* Custom-layer parameter dictionary entry: `parameters: [String : Any]`
 * (ProposalLayer.swift:65).  Keys and types are fixed by the converter,
 * Sources/maskrcnn/Python/Conversion/task.py:25-67 (intValue / doubleValue). */
typedef enum { MRCNN_PARAM_INT = 0, MRCNN_PARAM_DOUBLE = 1, MRCNN_PARAM_STRING = 2 } mrcnn_param_type;
typedef struct {
    const char* key;
    int32_t     type;    /* mrcnn_param_type */
    int64_t     i;
    double      d;
    const char* s;
} mrcnn_param;

/* ---------------------------------------------------------------------------------------------
 * MaskRCNNConfig.defaultConfig (Sources/Mask-RCNN-CoreML/MaskRCNNConfig.swift:10-18):
 * process-global URLs read by the layers at init/evaluate (ProposalLayer.swift:68,
 * TimeDistributedClassifierLayer.swift:41, TimeDistributedMaskLayer.swift:49).  Must be set before
 * the main model / ProposalLayer is created (Example/Source/AppDelegate.swift:18-20).
 * NULL clears.  Getters return NULL when unset; the pointer stays valid until the next set.
 * --------------------------------------------------------------------------------------------- */
MRCNN_API int mrcnn_config_set_anchors_path(const char* path);      /* anchorsURL                  */
MRCNN_API int mrcnn_config_set_classifier_path(const char* path);   /* compiledClassifierModelURL  */
MRCNN_API int mrcnn_config_set_mask_path(const char* path);         /* compiledMaskModelURL        */
MRCNN_API const char* mrcnn_config_get_anchors_path(void);
MRCNN_API const char* mrcnn_config_get_classifier_path(void);
MRCNN_API const char* mrcnn_config_get_mask_path(void);

/* ---------------------------------------------------------------------------------------------
 * The five MLCustomLayer plugins.  Core ML resolves them BY @objc CLASS NAME from the model spec
 * (task.py:27,39,48,53,59) and drives four methods; mrcnn_layer_* mirror them one to one:
 *
 *   init(parameters:)                 → mrcnn_layer_create      (ProposalLayer.swift:65, PyramidROIAlignLayer.swift:48,
 *                                                                DetectionLayer.swift:63, TimeDistributed*Layer.swift:18)
 *   setWeightData(_:)                 → mrcnn_layer_set_weight_data   (no-op in all five: ProposalLayer.swift:93)
 *   outputShapes(forInputShapes:)     → mrcnn_layer_output_shapes     (ProposalLayer.swift:97, PyramidROIAlignLayer.swift:65,
 *                                                                DetectionLayer.swift:94, TimeDistributedClassifierLayer.swift:26,
 *                                                                TimeDistributedMaskLayer.swift:26)
 *   evaluate(inputs:outputs:)         → mrcnn_layer_evaluate          (ProposalLayer.swift:103, PyramidROIAlignLayer.swift:79,
 *                                                                TimeDistributedClassifierLayer.swift:34, DetectionLayer.swift:107,
 *                                                                TimeDistributedMaskLayer.swift:39)
 *
 * class_name ∈ { "ProposalLayer", "PyramidROIAlignLayer", "TimeDistributedClassifierLayer",
 *                "DetectionLayer", "TimeDistributedMaskLayer" }.
 *
 * evaluate inputs/outputs per layer (all Float32):
 *   ProposalLayer                  in : probs (A,·,2…) contiguous (A,2); deltas (A,4)          out: rois, maxProposals rows of 4, row stride strides[0]
 *   PyramidROIAlignLayer           in : rois (n rows, stride strides[0]); 4 maps [·,·,C,H,W]   out: [n,1,C,pool,pool], row stride strides[0]
 *   TimeDistributedClassifierLayer in : pooled [n,1,C,7,7]                                      out: [n,1,1,1,6] rows (dy,dx,dh,dw,classId,score), row stride strides[2]
 *   DetectionLayer                 in : rois (n,4) row stride strides[0]; cls (n,6) contiguous  out: maxDetections rows of 6, row stride strides[0]
 *   TimeDistributedMaskLayer       in : pooled [D,1,C,14,14]; detections (D rows, strides[0])   out: [1,1,D,28,28], row stride strides[2]; rows the
 *                                        reference never writes (TimeDistributedMaskLayer.swift:58-89) are left untouched
 * --------------------------------------------------------------------------------------------- */
typedef struct mrcnn_layer mrcnn_layer;

MRCNN_API int mrcnn_layer_create(const char* class_name, const mrcnn_param* params, int n_params,
                                 mrcnn_layer** out_layer);
MRCNN_API int mrcnn_layer_set_weight_data(mrcnn_layer* layer, const void* const* blobs,
                                          const size_t* sizes, int n_blobs);
MRCNN_API int mrcnn_layer_output_shapes(mrcnn_layer* layer, const int64_t (*in_shapes)[5], int n_in,
                                        int64_t (*out_shapes)[5], int* n_out);
MRCNN_API int mrcnn_layer_evaluate(mrcnn_layer* layer, const mrcnn_tensor* inputs, int n_in,
                                   mrcnn_tensor* outputs, int n_out);
MRCNN_API void mrcnn_layer_destroy(mrcnn_layer* layer);

/* Stand-alone numerics helpers that are public in the reference:
 *   IOU(_:_:)  Sources/Mask-RCNN-CoreML/Utils.swift:232  (boxes as (y1,x1,y2,x2) floats; Double arithmetic, Float result).
 * Host-only (no GPU involved, as in the reference). */
MRCNN_API float mrcnn_iou(const float a_yxyx[4], const float b_yxyx[4]);

/* ---------------------------------------------------------------------------------------------
 * The three-model surface.  Xcode generates `MaskRCNN`, `Classifier`, `Mask` classes from the
 * .mlmodel files (Example/iOS Example.xcodeproj/project.pbxproj:25-28); the host uses
 * `MaskRCNN().model` (Example/Source/ViewController.swift:37) and reads outputs "detections" and
 * "mask" (task.py:70-72,87-89).  Here a model is a .mrcw artefact (see DESIGN.md "Artefacts").
 * --------------------------------------------------------------------------------------------- */
typedef enum { MRCNN_MODEL_MASKRCNN = 0, MRCNN_MODEL_CLASSIFIER = 1, MRCNN_MODEL_MASK = 2 } mrcnn_model_kind;
typedef struct mrcnn_model mrcnn_model;

/* Loads weights to the current HIP device, folds BatchNorm, repacks kernels, builds the static
 * schedule.  For MRCNN_MODEL_MASKRCNN the anchors / Classifier / Mask artefacts are taken from the
 * config singleton at load time (like ProposalLayer.init, ProposalLayer.swift:68), and loaded ONCE
 * (the reference re-loads the sub-models on every evaluate, TimeDistributedClassifierLayer.swift:41 —
 * deliberately not reproduced).  max_batch sizes the activation arena (images per predict call).
 * compute_dtype: MRCNN_DEFAULT — what a drop-in host passes (`MaskRCNN()` of ViewController.swift:37 names no precision): a MaskRCNN
 * artefact that carries stored split exponents ("split_exp.<group>" metadata, written by `convert --calibrate`) loads as MRCNN_F32X3
 * — fp32 tensors, every product exact, the mode bench.py's `value` is measured in — with those exponents applied; any other artefact
 * (no calibration stored; the stand-alone Classifier / Mask models) loads as MRCNN_F32.  mrcnn_model_get_int "compute_dtype" returns
 * the resolved mode, "compute_dtype_defaulted" 1 when it was chosen this way.  Explicit modes: MRCNN_F32 (exact-fp32 MFMA, fp32
 * activations — the parity baseline), MRCNN_F16 (fp16 activations and filters, fp32 accumulate, fp32 box path and outputs:
 * BASELINE configs[3]) or MRCNN_F32S (everything stays fp32 in memory; each convolution runs as TWO fp16
 * MFMA passes over a hi/lo split of its fp32 activations against the fp16 filters the artefact stores
 * (task.py:90), fp32 accumulate: products are exact, the split carries 22 of the 24 significand bits —
 * fp32-grade results at several times the fp32-MFMA rate.  Requires fp16-representable filters, which is
 * what the converter writes; an artefact with genuine fp32 filters is refused in this mode).  MRCNN_F32X3 is the same
 * with THREE parts — three MFMA passes instead of two.  The bound that holds: an activation with 0.5 <= |a| < 65504 is
 * represented exactly (its product with an fp16 filter is then exact and only the fp32 summation order differs from an fp32
 * engine); a smaller one is carried to 2^-25 ABSOLUTE, rounded to nearest (the third part reaches the fp16 subnormal
 * step; this also relies on the MFMA not flushing fp16 subnormals, which gfx950 does not), i.e. about 14 significant bits
 * at |a| = 1e-3.  An output is therefore off by at most 2^-25 * sum|w| beyond fp32 summation noise: invisible while a layer's
 * activations are O(1) or larger (every tensor of a BatchNorm-folded trunk), but unlike fp32 the RAW split is not scale-invariant
 * (tests/test_gpu_conv_kernels.py, profiles/r03_split_scale_curve.txt).  mrcnn_model_calibrate_split (below) removes the caveat:
 * a power-of-two exponent per tensor group, folded into the layers at no run-time cost, keeps every tensor's maximum in
 * [2^11, 2^12) — the mode is then fp32-grade for a checkpoint at ANY activation scale (tests/test_gpu_split_scale.py) and a
 * checkpoint whose raw activations would leave the fp16 range runs instead of tripping the watchdog.
 * End-to-end tolerance of MRCNN_F16 (BASELINE configs[3]; tests/test_gpu_fullsize.py::test_fp16_mode_end_to_end_bar, full size,
 * batch 8, against the fp32 CPU oracle): >= 95 % of the detections have a partner with the same class id and a box within 2e-3
 * (normalized coordinates), matched scores within 5e-4, matched masks within 3e-2; the fp32 modes' bars are 1e-4 / 1e-5 / 2e-4
 * with >= 99.9 % matched.
 * In MRCNN_F16, MRCNN_F32S and MRCNN_F32X3 every convolution watches its outputs for values leaving the fp16 range (|v| >= 65504,
 * which the next layer could not read; mrcnn_model_get_int key "range_overflows" counts the predicts it trips on).
 *   - Split modes (MRCNN_F32S / MRCNN_F32X3): such a predict is NOT failed — the reference's CPU path is fp32 activations x fp16 weights
 *     (Conversion/task.py:90) and has no such failure.  The batch, still resident on the device, is measured (one calibration pass),
 *     the split exponents are LOWERED to what it needs (never raised), and the batch is computed again before the call returns
 *     (key "range_recoveries"); mrcnn_maskrcnn_collect does the same for a pipelined batch.  Only an enqueue-only predict
 *     (mrcnn_maskrcnn_predict_async + mrcnn_model_check_range) leaves the re-run to the host.
 *   - MRCNN_F16 (fp16 tensors, inherently range-limited): the synchronous predict fails with MRCNN_ERR_UNSUPPORTED instead of
 *     returning saturated results. */
MRCNN_API int mrcnn_model_load(int kind, const char* path, int max_batch, int compute_dtype,
                               mrcnn_model** out_model);
MRCNN_API void mrcnn_model_destroy(mrcnn_model* model);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the model's own. */
MRCNN_API int mrcnn_model_set_stream(mrcnn_model* model, void* hip_stream);

/* Optional hipGraph replay of predict's launch sequence (captured on the second call at a given batch size;
 * ~200 launches per image batch).  Off by default (measured neutral on MI355X); on = 1 enables it,
 * on = 0 switches back to plain stream launches and frees the captured graphs; the environment variable
 * MRCNN_GRAPH=1 sets the default for new handles.  Replay is bypassed automatically while stage timing or the conv
 * profile is enabled, and when the caller is itself capturing the stream (the launches then join the caller's
 * graph).  mrcnn_model_get_int keys "graph_enabled" / "graph_launches" report the state. */
MRCNN_API int mrcnn_model_enable_graph(mrcnn_model* model, int on);

/* MaskRCNN.prediction(image:) — input `image` (task.py:70-75): RGB 8-bit, H×W = the model's
 * input_image_shape, interleaved (B,H,W,3).  The per-channel mean is subtracted on the GPU.
 * Outputs: `detections` (B, maxDetections, 6) rows (y1,x1,y2,x2,classId,score) normalized,
 * zero-padded; `mask` (B, maxDetections, 28, 28).  Batched predict is an extension (the reference
 * is batch 1).  memspace says where image/detections/masks live (host or device). */
MRCNN_API int mrcnn_maskrcnn_predict(mrcnn_model* model, const uint8_t* rgb, int batch, int height,
                                     int width, int memspace, float* detections, float* masks);
/* `.scaleFit` inside predict (VNCoreMLRequest.imageCropAndScaleOption = .scaleFit, EvaluateCommand.swift:152-157,
 * ViewController.swift:45): images of ANY size height×width (the same for the whole batch) are letterboxed — aspect-preserving
 * bilinear resize, centred, black borders: exactly mrcnn_letterbox_rgb's pixels — into the model's input size INSIDE the
 * pre-processing kernel; the results equal mrcnn_letterbox_rgb + mrcnn_maskrcnn_predict bit for bit.  Boxes come back normalized
 * in the letterboxed frame, like the reference's (EvaluateCommand.swift:203-248); mrcnn_unletterbox_boxes maps rows
 * (y1,x1,y2,x2,...) of `stride` floats back to the source image's normalized frame (host arithmetic, in place). */
MRCNN_API int mrcnn_maskrcnn_predict_scalefit(mrcnn_model* model, const uint8_t* rgb, int batch, int height, int width, int memspace,
                                              float* detections, float* masks);
MRCNN_API int mrcnn_unletterbox_boxes(float* detections, int64_t n, int64_t stride, int src_h, int src_w, int model_h, int model_w);
/* One predict over images of DIFFERENT sizes — what a host walking a directory of photos has (EvaluateCommand.swift:159-200: no two
 * consecutive COCO images share a size).  images[b] is RGB8 interleaved (height, width, 3), any size 1..32767 per side; every image
 * is letterboxed into the model's input with its OWN geometry inside ONE pre-processing launch (a per-image descriptor table on the
 * device; the letterboxed images are never materialised), so record b equals mrcnn_maskrcnn_predict_scalefit on image b alone, bit
 * for bit.  Outputs as predict_scalefit's: detections (batch, maxDetections, 6) normalized in the LETTERBOXED frame, masks (batch,
 * maxDetections, 28, 28), zero-padded.  memspace holds for every rgb pointer and both outputs; the table itself is host memory.
 * The images are copied to the device inside the call: the caller's buffers (and the table) only have to stay valid until it
 * returns.  Synchronous; never replayed from a captured graph; range recovery of the split modes works as in predict.
 * Errors: null table / null rgb -> MRCNN_ERR_INVALID; batch outside 1..max_batch or a side outside 1..32767 -> MRCNN_ERR_SHAPE;
 * the message names the index of the offending image.  mrcnn_paste_masks_source (below) turns the result into boxes and binary
 * masks in each image's own pixels. */
typedef struct { const uint8_t* rgb; int32_t height, width; } mrcnn_image;
MRCNN_API int mrcnn_maskrcnn_predict_images(mrcnn_model* model, const mrcnn_image* images, int batch, int memspace,
                                            float* detections, float* masks);
/* Pipelined host entry — the evaluate loop of EvaluateCommand.swift:167-179 (images handed over one call after the other, the
 * hand-over inside the per-image time) with the hand-over of batch i + 1 OVERLAPPED with the computation of batch i:
 *   mrcnn_maskrcnn_submit   copies a batch of host images (pinned memory makes the copy asynchronous) on the handle's copy
 *                           stream into one of two staging buffers and enqueues its predict behind the copy; returns at once.
 *                           At most two submissions may be in flight.
 *   mrcnn_maskrcnn_collect  waits for the OLDEST submission and copies its records to the host buffers (*batch = its size);
 *                           reports that batch's range-watchdog status like the synchronous predict.
 * The loop:  submit(b0); for i: submit(b[i+1]); collect(results of b[i]).   Results are bit-identical to
 * mrcnn_maskrcnn_predict's (the same launches on the same stream); do not interleave it with the synchronous entry while a
 * submission is in flight.  examples/maskrcnn_predict_stream.c is this loop as a plain-C host. */
MRCNN_API int mrcnn_maskrcnn_submit(mrcnn_model* model, const uint8_t* rgb_host, int batch, int height, int width);
MRCNN_API int mrcnn_maskrcnn_collect(mrcnn_model* model, float* detections_host, float* masks_host, int* batch);
/* Same, but only enqueues on the model's stream (no synchronisation); device buffers only. */
MRCNN_API int mrcnn_maskrcnn_predict_async(mrcnn_model* model, const uint8_t* rgb, int batch, int height,
                                           int width, float* detections, float* masks);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU of a node; new functionality of the MI355X build — the reference runs one image on one
 * device, the host loop that would drive this is Sources/maskrcnn/EvaluateCommand.swift:146-179).  A batch is split into
 * contiguous blocks of images (blocks differ by at most one image), every rank loads the same artefacts and predicts
 * its block, and ONE ncclAllGather over RCCL/xGMI — issued on the model's stream — hands every rank the fixed-size,
 * zero-padded records of the whole batch in image order:
 *     record = detections (maxDetections × 6 f32) ‖ mask (maxDetections × 28 × 28 f32)     316 000 B at the defaults.
 * Per-image results do not depend on the world size (tests).  RCCL is bound at run time (librccl.so.1).
 *   mrcnn_dist_unique_id   rank 0 creates the 128-byte rendezvous id; the HOST ships it to the other ranks (file, env, pipe)
 *   mrcnn_dist_init        joins the communicator on the calling thread's current HIP device
 *   mrcnn_dist_shard       [begin, end) of `rank` in a batch of `global_batch` images (host arithmetic, no GPU needed)
 *   mrcnn_dist_record_floats  floats per image record
 *   mrcnn_dist_all_gather_records  local results (end-begin images, `memspace`) → all `global_batch` results (`memspace`)
 *   mrcnn_maskrcnn_predict_sharded  the whole step: every rank passes the SAME global batch (global_batch, H, W, 3) and
 *                          receives detections (global_batch, maxDet, 6) / masks (global_batch, maxDet, 28, 28)
 * A rank never skips the collective: what it contributes is a SLOT = its records zero-padded to the largest shard + a
 * 4-word trailer [status, images, 0, 0].  A rank whose local predict failed (HIP error, the data-dependent fp16-range
 * watchdog) sends zeroed records with its status, and EVERY rank returns that status after the gather (its own message on
 * the failing rank, "rank r failed ..." on the others) — nobody is left blocked in ncclAllGather.
 *   mrcnn_dist_all_gather_records_async / mrcnn_dist_wait  the same exchange (device buffers only) issued on the handle's
 *                          own stream behind the model's stream: returns at once, the model's NEXT predict overlaps it (the
 *                          model's stream only waits until the results are packed before it may overwrite them);
 *                          mrcnn_dist_wait joins it and reports remote failures.  One exchange in flight per handle.
 *   mrcnn_dist_plan        host arithmetic of one exchange, no GPU needed: table[4*r + {0,1,2,3}] = {first image, end image,
 *                          float offset of rank r's slot in the gathered buffer, record floats rank r contributes};
 *                          *slot_floats = floats per slot
 *   mrcnn_dist_simulate_host  the pack -> concatenate (what ncclAllGather does) -> unpack code of the device path run on
 *                          host buffers for all `world` ranks in one process (detections[r] / masks[r] = rank r's local
 *                          results, status[r] optional): the seam through which the layout is tested at world sizes the
 *                          build machine does not have.  status[r] == MRCNN_DIST_ABORTED models a rank that could not even
 *                          enqueue a zeroed slot and tore the communicator down (ncclCommAbort): the call fails with
 *                          MRCNN_ERR_HIP — what every peer's ncclAllGather does then — and writes nothing */
#define MRCNN_DIST_ABORTED (-1)
typedef struct mrcnn_dist mrcnn_dist;
MRCNN_API int mrcnn_dist_unique_id(uint8_t* id128);
MRCNN_API int mrcnn_dist_init(int rank, int world, const uint8_t* id128, mrcnn_dist** out);
MRCNN_API void mrcnn_dist_destroy(mrcnn_dist* dist);
MRCNN_API int mrcnn_dist_shard(int global_batch, int world, int rank, int* begin, int* end);
MRCNN_API int64_t mrcnn_dist_record_floats(int max_detections, int mask_size);
MRCNN_API int mrcnn_dist_all_gather_records(mrcnn_dist* dist, mrcnn_model* model, const float* detections, const float* masks,
                                            int global_batch, int memspace, float* out_detections, float* out_masks);
MRCNN_API int mrcnn_maskrcnn_predict_sharded(mrcnn_dist* dist, mrcnn_model* model, const uint8_t* rgb, int global_batch,
                                             int height, int width, int memspace, float* detections, float* masks);
MRCNN_API int mrcnn_dist_all_gather_records_async(mrcnn_dist* dist, mrcnn_model* model, const float* detections, const float* masks,
                                                  int global_batch, float* out_detections, float* out_masks);
MRCNN_API int mrcnn_dist_wait(mrcnn_dist* dist);
/* Range recoveries seen by the LAST completed exchange of mrcnn_maskrcnn_predict_sharded (split modes; §"scale-aware split" below): every rank's
 * slot carries, beside its status word, how many times its local predict lowered its split exponents in that call.  *ranks = how many ranks
 * did (0: every rank still holds the exponent vector it was given), per_rank[r] (optional, `world` entries) = rank r's count.  A rank that
 * recovered computes later images with other exponents than its peers: a job that wants per-image results independent of the rank then takes
 * the vector with the LOWEST exponents (mrcnn_model_get_split_exponents on the ranks that recovered, element-wise minimum — the host's own
 * all-reduce or the same record exchange) and gives it to every rank (mrcnn_model_set_split_exponents).  Identical on every rank, no GPU work. */
MRCNN_API int mrcnn_dist_recovered(mrcnn_dist* dist, int32_t* per_rank, int* ranks);
/* Which RCCL this library bound (dist.hip binds it at run time): 1 = the copy the process had already mapped (e.g. the one
 * PyTorch ships under the soname librccl.so.1 — taken first, so that a process holds ONE RCCL), 0 = its own dlopen of
 * librccl.so.1, -1 = RCCL could not be loaded.  Loads RCCL when it is not bound yet; needs no GPU. */
MRCNN_API int mrcnn_dist_rccl_shared(void);
MRCNN_API int mrcnn_dist_plan(int global_batch, int world, int max_detections, int mask_size, int64_t* table, int64_t* slot_floats);
MRCNN_API int mrcnn_dist_simulate_host(int world, int global_batch, int max_detections, int mask_size, const float* const* detections,
                                       const float* const* masks, const int32_t* status, float* out_detections, float* out_masks,
                                       int32_t* status_out);

/* Classifier.prediction(feature_map:) (task.py:106-113): feature_map (n,256,7,7) CHW →
 * probabilities (n, numClasses), bounding_boxes (n, numClasses*4) class-major. */
MRCNN_API int mrcnn_classifier_predict(mrcnn_model* model, const float* feature_map, int n, int memspace,
                                       float* probabilities, float* bounding_boxes);
/* Mask.prediction(feature_map:) (task.py:94-101): feature_map (n,256,14,14) CHW → masks (n,numClasses,28,28). */
MRCNN_API int mrcnn_mask_predict(mrcnn_model* model, const float* feature_map, int n, int memspace,
                                 float* masks);

/* Introspection: "num_classes", "image_height", "image_width", "max_proposals", "max_detections", "num_anchors",
 * "pre_nms_max_proposals", "pre_nms_count" (= min(num_anchors, pre_nms_max_proposals)), "mask_size" (side of the
 * square masks predict returns: 2 × the mask pool size = 28), "max_batch", "compute_dtype", "range_overflows", "range_recoveries",
 * "graph_enabled", "graph_launches", "gpu_busy_us" / "predict_calls" (GPU time between the first and the last command of
 * the synchronous predicts of this handle, HIP events on the model's stream, and their count); any other key is looked up in
 * the artefact's integer metadata. */
MRCNN_API int mrcnn_model_get_int(mrcnn_model* model, const char* key, int64_t* value);

/* Debug taps for parity tests: copies a named intermediate of the last predict (image b) to a host
 * buffer of `capacity` floats and reports its element count.  Names: "rpn_probs" (A,2),
 * "rpn_deltas" (A,4), "C1" (H/4,W/4,64 NHWC: the pooled stem output), "C2".."C5" (the backbone stages' outputs, NHWC,
 * 256 / 512 / 1024 / 2048 channels), "P2".."P5" (H,W,256 NHWC), "topk_idx" (int32 stored as float-exact values),
 * "boxes_sorted" (n,4), "rois" (maxProposals,4), "pooled" (maxProposals,7,7,256 NHWC),
 * "cls_probs" (maxProposals,nc), "cls_bbox" (maxProposals,nc*4), "cls6" (maxProposals,6),
 * "detections" (maxDetections,6), "pooled_mask" (maxDetections,14,14,256 NHWC), "mask" (maxDetections,784),
 * "keep_count" (1), "mask_row_flags" (maxDetections: the mask layer's removeZeros predicate per detection row). */
MRCNN_API int mrcnn_model_read_tensor(mrcnn_model* model, const char* name, int image_index,
                                      float* host_dst, int64_t capacity, int64_t* count);

/* fp16-range watchdog for the enqueue-only path: mrcnn_maskrcnn_predict reports an activation that left the fp16
 * range (MRCNN_F16 / MRCNN_F32S / MRCNN_F32X3) as MRCNN_ERR_UNSUPPORTED when it synchronises; _predict_async cannot.
 * Call this after the stream work of an async predict has been ordered before the caller's consumer: it
 * synchronises the model's stream and sets *tripped = 1 when the LAST predict's results are not valid
 * (counted in "range_overflows" like the synchronous path).  Always 0 in MRCNN_F32. */
MRCNN_API int mrcnn_model_check_range(mrcnn_model* model, int* tripped);

/* ---------------------------------------------------------------------------------------------
 * Scale-aware split — what makes MRCNN_F32X3 / MRCNN_F32S fp32-grade at ANY activation scale.
 * The split modes carry an fp32 activation exactly while 0.5 <= |a| < 65504 and to 2^-25 ABSOLUTE below, so a checkpoint
 * whose tensors sit at 1e-3 would lose accuracy (and one at 1e5 would trip the range watchdog) where the reference's CPU path
 * — fp32 activations, fp16 weights (Conversion/task.py:90) — is scale-free.  Every tensor a split convolution reads belongs to
 * a GROUP with an exponent e: it is STORED as 2^e * value, an exact operation folded at no run-time cost into the producer's
 * BatchNorm scale / shift and undone in the consumer's (ReLU, max-pool, the bilinear sampler and the residual add commute).
 * With every e = 0 (the state after mrcnn_model_load) nothing changes.
 *   mrcnn_model_calibrate_split  one predict on the given images collects max |a| per group, picks e with max |a| * 2^e in
 *                          [2^11, 2^12) (16x head room under the fp16 range, everything above 2^-13 of the maximum exact), and a
 *                          second predict verifies the choice and counts the inputs a split still cannot carry exactly;
 *                          apply = 0 only diagnoses (exponents untouched).  Outputs, taps and every stage after the convolutions
 *                          are in true scale either way; results are bit-identical for any batch split as before.
 *   mrcnn_model_get_int    "split_small_inputs" (non-zero inputs below 2^-8 of their tensor's maximum), "split_inexact_inputs"
 *                          (non-zero stored inputs below 0.5: carried to 2^-25 absolute, i.e. <= 2^-36 of the maximum once
 *                          calibrated), "split_inputs_counted", "split_min_exponent" / "split_max_exponent", "split_calibrated",
 *                          "split_groups" — next to "range_overflows"
 *   mrcnn_model_split_group_stat   per group: name, exponent, max |a|, the three counters
 *   mrcnn_model_get/set_split_exponents   the exponents as a vector (one per group, 0 for the groups fp32 arithmetic consumes):
 *                          a sharded job calibrates on one rank — or offline — and sets the same vector on every rank.
 *   stored exponents       `python -m mask-rcnn-coreml_amd.convert ... --calibrate <images>` writes the vector into MaskRCNN.mrcw
 *                          ("split_exp.<group>" metadata); mrcnn_model_load applies it in the split modes, so the drop-in
 *                          MaskRCNN().prediction(image) (ViewController.swift:37) runs calibrated without any extra call
 *                          ("split_exponents_from_artefact" = 1, "split_calibrated" = 1).
 *   range recovery         a batch that leaves the calibrated range lowers the exponents it needs and is computed again inside the
 *                          call (see mrcnn_model_load above; "range_recoveries").  Later batches use the lowered vector: a sharded job
 *                          that wants bit-equal results across ranks after a recovery re-distributes it with get / set.
 * MRCNN_F32 and MRCNN_F16 models return MRCNN_ERR_UNSUPPORTED from calibrate / set. */
typedef struct mrcnn_split_group_stat {
    char    name[48];
    int32_t exponent;
    int32_t fixed;            /* 1: consumed by fp32 arithmetic (logits, deltas, probabilities): exponent stays 0 */
    float   absmax;           /* max |a| of the true values over the calibration images */
    int64_t small_inputs, inexact_inputs, inputs_counted;
} mrcnn_split_group_stat;
MRCNN_API int mrcnn_model_calibrate_split(mrcnn_model* model, const uint8_t* rgb, int batch, int height, int width, int memspace, int apply);
MRCNN_API int mrcnn_model_split_group_stat(mrcnn_model* model, int index, mrcnn_split_group_stat* out);
MRCNN_API int mrcnn_model_get_split_exponents(mrcnn_model* model, int32_t* exponents, int capacity, int* count);
MRCNN_API int mrcnn_model_set_split_exponents(mrcnn_model* model, const int32_t* exponents, int count);

/* PyramidROIAlign (PyramidROIAlignLayer.swift:79-181) on the engine's own layout: four NHWC maps (H_l, W_l, C),
 * dtype MRCNN_F32 or MRCNN_F16; rois rows (y1,x1,y2,x2,...) of `roi_stride` floats; out (n_rois, pool, pool, C)
 * in the maps' dtype.  row_flags (optional, n_rois int32): the removeZeros predicate the mask layer applies to a
 * pooled row (TimeDistributedClassifierLayer.swift:116-127: kept iff every element != 0) evaluated on the fp32
 * samples BEFORE the store rounds them — in fp16 a tiny non-zero sample would otherwise flush to zero and drop a
 * valid detection.  This is what the fused engine uses; the stand-alone MLCustomLayer entry takes CHW fp32.
 * channels % 4 == 0.  MRCNN_DEVICE: the kernel reads the maps and writes `out` where they lie with 16-byte vector accesses — maps and out
 * 16-byte aligned (any allocation is; a slice must start on a multiple of 16 bytes). */
MRCNN_API int mrcnn_roi_align_nhwc(const void* const maps[4], const int heights[4], const int widths[4], int channels,
                                   int dtype, const float* rois, int64_t roi_stride, int n_rois, int pool,
                                   double image_w, double image_h, int memspace, void* out, int32_t* row_flags);

/* Per-stage GPU time of the last predict in milliseconds (HIP events on the model's stream).
 * Stage names mirror the reference's os_signpost intervals (ProposalLayer.swift:105-194 etc.):
 * "Trunk", "Proposal-Eval", "PyramidROIAlign-Eval", "TimeDistributedClassifierLayer-Eval",
 * "Detection-Eval", "PyramidROIAlign-Eval-Mask", "TimeDistributedMask-Eval".
 * Only collected after mrcnn_model_enable_timing(model, 1). */
MRCNN_API int mrcnn_model_enable_timing(mrcnn_model* model, int on);
MRCNN_API int mrcnn_model_stage_ms(mrcnn_model* model, const char* stage, float* ms);

/* Test and measurement entry points (the convolution micro-benchmark hook, the per-kernel live profile, the
 * single-convolution parity entry and the process-wide kernel-selection knobs) are exported by the same library but
 * declared in include/maskrcnn_hip_test.h: they are not part of the drop-in surface — nothing in the reference's
 * interface (ProposalLayer.swift:52-103, MaskRCNNConfig.swift:10-18) is a debug knob. */

/* ---------------------------------------------------------------------------------------------
 * Result decoding — Detection.detectionsFromFeatureValue (Sources/Mask-RCNN-CoreML/
 * Detection.swift:23-62) and maskFromFeatureValue (:64-99).  Host-side, like the reference.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t index;        /* row in the detections array                       (Detection.swift:17) */
    double  x, y, w, h;   /* boundingBox CGRect(x: x1, y: y1, width, height)   (Detection.swift:55) */
    int64_t class_id;
    double  score;
} mrcnn_detection;

/* Keeps rows with score > 0.7 (Detection.swift:38).  Writes at most `capacity` records; returns the
 * number kept in *count. */
MRCNN_API int mrcnn_detections_decode(const float* detections, int64_t n_rows, int64_t row_stride,
                                      mrcnn_detection* out, int64_t capacity, int64_t* count);
/* Anchors on demand (the reference's own TODO, MaskRCNNConfig.swift:14): writes the (A,4) float32
 * normalized (y1,x1,y2,x2) anchors that the converter dumps to anchors.bin (task.py:173-176) for the
 * default scales (32..512), ratios (0.5,1,2) and strides (4..64).  Host code.  Call with out = NULL to
 * query *count = A. */
MRCNN_API int mrcnn_generate_anchors(int image_h, int image_w, float* out, int64_t capacity, int64_t* count);

/* Letterbox: Vision's `.scaleFit` (EvaluateCommand.swift:157, ViewController.swift:45) on
 * the GPU — RGB8 (h,w,3) resized with preserved aspect ratio (bilinear, half-pixel centres) and centred in
 * an (H,W,3) canvas with black borders.  _geometry returns the content size and offsets (host arithmetic)
 * so that callers can map normalized boxes back to the source image. */
MRCNN_API int mrcnn_letterbox_geometry(int h, int w, int H, int W, int* nh, int* nw, int* pad_y, int* pad_x);
MRCNN_API int mrcnn_letterbox_rgb(const uint8_t* src, int h, int w, int memspace, uint8_t* dst, int H, int W);

/* JPEG: compressed bytes in (the reference reads `<dataset dir>/<file_name>`, EvaluateCommand.swift:159-200, and every COCO file is a
 * JPEG).  The serial part — marker parsing, Huffman decoding — runs on the host; dequantisation, the 8x8 inverse DCT, chroma
 * upsampling and YCbCr -> RGB run in two launches for the whole batch, and the decoded RGB8 never exists in host memory.
 * The output is DEFINED as what libjpeg / libjpeg-turbo produce with their defaults (JDCT_ISLOW, fancy upsampling), byte for byte.
 *   decoded:     baseline sequential DCT (SOF0), 8-bit, Huffman, one interleaved scan; 1 component (grey, replicated to RGB) or 3
 *                (YCbCr) sampled 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2); 8- and 16-bit quantisation tables; any DHT; restart intervals;
 *                APPn / COM are skipped; sides 1..32767
 *   refused:     progressive, arithmetic, lossless, 12-bit, 4 components, an Adobe transform other than YCbCr, other sampling
 *                factors, multi-scan sequential files -> MRCNN_ERR_UNSUPPORTED, the message names what was found
 *   damaged or truncated stream -> MRCNN_ERR_IO.  No input, however malformed, is read or written out of bounds.
 * A file is ALWAYS host memory.  _info and _decode_host are host code and need no GPU; _decode_host is the whole pipeline in scalar C++,
 * the definition the device entry is held to (rgb: height*width*3 bytes; capacity too small -> MRCNN_ERR_SHAPE).
 * _decode_batch: files of different sizes; image b's height*width*3 bytes go to out_rgb + out_offsets[b] (`memspace` is out_rgb's;
 * offsets are bytes, multiples of 16, the ranges must not overlap, bytes no image covers are left untouched — the conventions of
 * mrcnn_render_detections_source); heights / widths (host, `batch` entries) are outputs.  Every file is validated first, before anything
 * is written; an error names the index of the offending file.  Entropy decoding runs on min(batch, 8) threads of the call.
 * Errors: null pointer, bad offset -> MRCNN_ERR_INVALID; batch outside 1..MRCNN_JPEG_MAX_BATCH -> MRCNN_ERR_SHAPE; no gfx950 device
 * -> MRCNN_ERR_HIP from the two device entries (no CPU fallback).
 * mrcnn_maskrcnn_predict_jpegs = _decode_batch into staging the model owns + mrcnn_maskrcnn_predict_images on it, bit for bit
 * (`memspace` is that of detections and masks; batch 1..max_batch). */
#define MRCNN_JPEG_MAX_BATCH 1024
typedef struct { const uint8_t* data; int64_t length; } mrcnn_jpeg;
MRCNN_API int mrcnn_jpeg_info(const uint8_t* data, int64_t length, int32_t* height, int32_t* width, int32_t* components, int32_t* h_samp,
                              int32_t* v_samp);
MRCNN_API int mrcnn_jpeg_decode_host(const uint8_t* data, int64_t length, uint8_t* rgb, int64_t capacity);
MRCNN_API int mrcnn_jpeg_decode_batch(const mrcnn_jpeg* files, int batch, int memspace, uint8_t* out_rgb, const int64_t* out_offsets,
                                      int32_t* heights, int32_t* widths);
MRCNN_API int mrcnn_maskrcnn_predict_jpegs(mrcnn_model* model, const mrcnn_jpeg* files, int batch, int memspace, float* detections,
                                           float* masks, int32_t* heights, int32_t* widths);
/* The same two entries with the ENTROPY stage chosen by the caller.  MRCNN_JPEG_ENTROPY_HOST is what the entries above run.
 * MRCNN_JPEG_ENTROPY_DEVICE (opt-in) decodes the Huffman streams on the device too — self-synchronising parallel decoding
 * (kernels_jpeg_entropy.hip): the files' bytes, not their coefficients, are uploaded, and the host does a marker scan only.  A file the
 * device's verdict does not call clean (a damaged stream, fill bytes before a marker, a stream that does not resynchronise within the
 * round cap) goes through the host decoder after all, whose coefficients, status and message are then the call's: for every input the
 * bytes, the status and the message equal MRCNN_JPEG_ENTROPY_HOST's.  LIMIT: the number of synchronisation launches is set from the files'
 * sizes and capped (4 with the 128-byte units): an intact file in which a wrong decoder state survives more than 64 KB of stream is
 * given to the host decoder too — same result, the host's speed.  Any other `entropy` -> MRCNN_ERR_INVALID. */
enum { MRCNN_JPEG_ENTROPY_HOST = 0, MRCNN_JPEG_ENTROPY_DEVICE = 1 };
MRCNN_API int mrcnn_jpeg_decode_batch_on(const mrcnn_jpeg* files, int batch, int memspace, int entropy, uint8_t* out_rgb,
                                         const int64_t* out_offsets, int32_t* heights, int32_t* widths);
MRCNN_API int mrcnn_maskrcnn_predict_jpegs_on(mrcnn_model* model, const mrcnn_jpeg* files, int batch, int memspace, int entropy,
                                              float* detections, float* masks, int32_t* heights, int32_t* widths);

/* JPEG: files out — the rendered overlays of mrcnn_render_detections_source (or any RGB8 image) leave as baseline JPEG files, and the
 * whole encoder runs on the device: colour conversion, chroma downsampling, forward DCT, quantisation, Huffman coding (code lengths
 * counted per block and scanned, then every block's bits written at once) and byte stuffing.  Only the files' bytes cross back.
 *   the file:    baseline sequential (SOF0), 8-bit, one interleaved scan; SOI, JFIF APP0 (1.1, density 1:1, no units), DQT, SOF0, DHT,
 *                SOS, scan, EOI.  Quantisation: Annex K's tables scaled by libjpeg's quality rule (scale = 5000/q below 50, else
 *                200 - 2q; entry = (base*scale + 50)/100 clamped to 1..255).  Huffman: the four standard Annex K tables.
 *   left out:    restart markers, optimised Huffman tables, progressive scans.
 *   the samples: libjpeg's default compressor in integers — 16-bit fixed-point RGB -> YCbCr, box chroma downsampling with libjpeg's
 *                alternating bias, edges replicated, level shift -128, the jfdctint (ISLOW) forward DCT, round-half-away division by 8q.
 *                Blocks that exist only as MCU padding are ordinary blocks of replicated samples (libjpeg writes DC-only dummies), so the
 *                bytes differ from libjpeg's while every visible pixel decodes to the same value.
 * sampling: MRCNN_JPEG_444 / _422 (h2v1) / _420 (h2v2) / _GREY (one component: the Y above).  quality 1..100.  sides 1..32767.
 * _encode_host is plain scalar C++, needs no GPU and is the DEFINITION: _encode_batch returns the same bytes, byte for byte.  *length is
 * always the size needed; out = NULL with capacity = 0 measures; capacity too small -> MRCNN_ERR_SHAPE and nothing is written.
 * _encode_batch: images of different sizes, as given to mrcnn_maskrcnn_predict_images or left by mrcnn_render_detections_source;
 * `memspace` is that of the rgb pointers (any alignment); the files are ALWAYS host memory: file b is out[file_offsets[b] ..
 * file_offsets[b + 1]), back to back.  file_offsets (host, batch + 1 entries) is always written.  file_offsets[batch] > capacity ->
 * MRCNN_ERR_SHAPE naming the capacity needed, with out untouched; capacity 0 with out = NULL is the size query.  Only the used bytes
 * are copied from the device, and the number of launches does not depend on batch.
 * Errors (the message names the index of the offending image), all raised before the device is touched: null pointer, unknown sampling
 * or memspace -> MRCNN_ERR_INVALID; a side outside 1..32767, quality outside 1..100, batch outside 1..MRCNN_JPEG_MAX_BATCH ->
 * MRCNN_ERR_SHAPE.  No gfx950 device -> MRCNN_ERR_HIP (no CPU fallback). */
enum { MRCNN_JPEG_444 = 0, MRCNN_JPEG_422 = 1, MRCNN_JPEG_420 = 2, MRCNN_JPEG_GREY = 3 };
MRCNN_API int mrcnn_jpeg_encode_host(const uint8_t* rgb, int height, int width, int quality, int sampling, uint8_t* out, int64_t capacity,
                                     int64_t* length);
MRCNN_API int mrcnn_jpeg_encode_batch(const mrcnn_image* images, int batch, int memspace, int quality, int sampling, uint8_t* out,
                                      int64_t capacity, int64_t* file_offsets /* batch + 1 */);

/* PNG: files out — the label images leave as lossless files: the int16 maps of mrcnn_instance_map_source and the uint8 mask planes of
 * mrcnn_paste_masks_source (JPEG cannot carry an id).  The deflate stream is made on the device: the bits of every token counted per
 * block and scanned, then every token written at once; only the files' bytes cross back, and no codec is linked.
 *   the formats: MRCNN_PNG_GREY8     pixels = uint8, height x width, row-major -> colour type 0, depth 8, the values as they are.
 *                MRCNN_PNG_INSTANCE  pixels = int16, height x width (what mrcnn_instance_map_source leaves) -> colour type 3 (palette),
 *                                    depth 8: index = v + 1 for v in -1 .. rows - 1, any other value index 0.  rows in 1..255.  PLTE has
 *                                    rows + 1 entries: entry 0 is (0,0,0), entry k >= 1 palette[(k-1) % 4] of mrcnn_render_detections_source
 *                                    (red, blue, green, yellow); tRNS is one byte, 0: "no detection" is transparent.  The file is the
 *                                    exact id map (index - 1) and a coloured overlay any viewer shows.
 *   the file:    signature, IHDR, [PLTE, tRNS], ONE IDAT, IEND.  Raw stream R: per scanline a filter byte 0 and the width sample
 *                bytes, N = height (width + 1).  IDAT = 78 01, a deflate stream, Adler-32 of R.  R is cut into blocks of
 *                MRCNN_PNG_BLOCK_BYTES raw bytes, each one fixed-Huffman block (BFINAL on the last), bit-contiguous, the last byte
 *                zero-padded.  Tokens (zlib's Z_RLE matcher, distance 1 only), for a block [b0, b1) and p from b0: n = the number of
 *                k >= 0 with R[p+k] == R[p+k-1], counted up to min(258, b1 - p), 0 at p = 0; n >= 3 -> (length n, distance 1), p += n;
 *                else the literal R[p], p += 1.
 *   left out:    RGB8, 16-bit samples, row filters other than 0 (they gain nothing on label data under this matcher), dynamic Huffman
 *                tables, interlacing, decoding.  Photographs come out larger than raw with fixed codes: pictures have the JPEG entries.
 * _encode_host is plain sequential C++, needs no GPU and is the DEFINITION: _encode_batch returns the same bytes, byte for byte.  *length
 * is always the size needed; out = NULL with capacity = 0 measures; capacity too small -> MRCNN_ERR_SHAPE and nothing is written.
 * _encode_batch: images of different sizes, all of one format; `memspace` is that of the pixel pointers (natural alignment of the sample
 * type); the files are ALWAYS host memory: file b is out[file_offsets[b] .. file_offsets[b + 1]), back to back.  file_offsets (host,
 * batch + 1 entries) is always written.  file_offsets[batch] > capacity -> MRCNN_ERR_SHAPE naming the capacity needed, with out
 * untouched; capacity 0 with out = NULL is the size query.  Only the used bytes are copied from the device (IDAT's CRC-32 is the host's,
 * filled in after the copy), and the number of launches does not depend on batch.  rows is ignored for MRCNN_PNG_GREY8.
 * Errors (the message names the index of the offending image), all raised before the device is touched: null pointer, unknown format
 * or memspace -> MRCNN_ERR_INVALID; a side outside 1..32767, rows outside 1..255 for MRCNN_PNG_INSTANCE, batch outside
 * 1..MRCNN_PNG_MAX_BATCH -> MRCNN_ERR_SHAPE.  No gfx950 device -> MRCNN_ERR_HIP from _encode_batch (no CPU fallback). */
enum { MRCNN_PNG_GREY8 = 0, MRCNN_PNG_INSTANCE = 1 };
#define MRCNN_PNG_BLOCK_BYTES 4096
#define MRCNN_PNG_MAX_BATCH 1024 /* the 100 mask planes of several images fit one call */
typedef struct { const void* pixels; int32_t height, width; } mrcnn_png_source;
MRCNN_API int mrcnn_png_encode_host(const void* pixels, int height, int width, int format, int rows, uint8_t* out, int64_t capacity,
                                    int64_t* length);
MRCNN_API int mrcnn_png_encode_batch(const mrcnn_png_source* images, int batch, int memspace, int format, int rows, uint8_t* out,
                                     int64_t capacity, int64_t* file_offsets /* batch + 1 */);

/* Mask paste: per-instance 28×28 sigmoid masks → full-resolution binary masks
 * (n, image_h, image_w) uint8 {0,1}: resize to the detection's box and threshold.  Replaces what the
 * example app does with CoreGraphics when drawing (Example/Source/DetectionRenderer.swift:13-24).
 * Box pixels = round-half-even(y*(H-1)) with +1 on the far edge (Matterport denorm_boxes), bilinear
 * with half-pixel centres, `>= threshold`; rows with score <= 0 give empty masks. image_w % 4 == 0. */
MRCNN_API int mrcnn_paste_masks(const float* detections, int64_t det_stride, const float* masks, int n, int mask_size,
                                int image_h, int image_w, float threshold, int memspace, uint8_t* out);
/* The same for a batch of images of DIFFERENT sizes, in each image's own pixels — the way back from mrcnn_maskrcnn_predict_images.
 * detections (batch, rows, 6) / masks (batch, rows, mask_size, mask_size) are what that call returned (rows = maxDetections), heights
 * / widths the sizes of the source images, model_h / model_w the model's input size.  For image b, row i:
 *   detections_src (batch, rows, 6)  the row with its box mapped to the SOURCE frame exactly as mrcnn_unletterbox_boxes(..., heights[b],
 *                                    widths[b], model_h, model_w) maps it (all-zero rows stay all-zero; class id and score copied)
 *   out + out_offsets[b] + i*h_b*w_b the h_b × w_b uint8 {0,1} mask mrcnn_paste_masks gives for that mapped box at image_h = h_b,
 *                                    image_w = w_b.  ANY width (no `% 4` rule here).
 * out_offsets: batch byte offsets, each a multiple of 16 (the planes of different images must not overlap); bytes of `out` that no
 * plane covers are left untouched.  memspace holds for detections, masks, detections_src and out; heights, widths and out_offsets
 * are host arrays.  The un-letterbox runs on the device and one launch pastes the whole batch. */
MRCNN_API int mrcnn_paste_masks_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                       const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                       int memspace, float* detections_src, uint8_t* out, const int64_t* out_offsets);
/* COCO run-length encoding (RLE) of the masks mrcnn_paste_masks_source would paste, without pasting them: the same arguments up to
 * detections_src, and for image b, row i (k = b*rows + i) the h_b x w_b plane of that call encoded as COCO does — pixels in
 * column-major order (p = x*h + y), counts[0] = the number of leading zeros (0 when pixel (0,0) is set), then alternating lengths of
 * runs of ones and zeros, summing to h*w; a row that pastes nothing is the single run [h*w].
 *   counts + run_offsets[k] .. counts + run_offsets[k+1]   the run lengths of row k (all rows back to back)
 *   run_offsets (batch*rows + 1), areas (batch*rows: the number of set pixels), bboxes_xywh (batch*rows*4: the tight box x, y, w, h of
 *   the set pixels, 0,0,0,0 for an empty mask) and detections_src are ALWAYS written; areas / bboxes_xywh may be NULL.
 * If run_offsets[batch*rows] > capacity the call returns MRCNN_ERR_SHAPE, the message names the capacity needed and counts is not
 * written (capacity = 0 with counts = NULL is the size query).  memspace holds for detections, masks, detections_src, counts,
 * run_offsets, areas and bboxes_xywh; heights and widths are host arrays.  With MRCNN_HOST only the used part of counts is copied. */
MRCNN_API int mrcnn_masks_rle_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                     const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                     int memspace, float* detections_src, uint32_t* counts, int64_t capacity, int64_t* run_offsets,
                                     uint32_t* areas, int32_t* bboxes_xywh);
/* Drawing (Example/Source/DetectionRenderer.swift:13-88: each 28×28 mask stretched over its box and filled in one of four colours,
 * the box stroked three pixels wide, everything over the photo) — for a batch of images of DIFFERENT sizes, in each image's own
 * pixels, straight from the 28×28 masks: the rows × h × w planes of mrcnn_paste_masks_source are never written.  Both entries are
 * defined by that call and nothing else.  For image b (h_b × w_b) and row i: box_i = (y1, x1, y2, x2), the pixel box of the mapped
 * row (round-half-even of y*(h_b-1), +1 on the far edge, which is exclusive; empty for a row that pastes nothing), P_i = the plane
 * mrcnn_paste_masks_source pastes for the row at `threshold`.  Row i is DRAWN if its score > min_score and box_i is not empty;
 * padding rows and rows with score <= 0 are never drawn, whatever min_score is.
 *
 * mrcnn_instance_map_source — DetectionRenderer.swift:13-24 without the colours: which detection owns a pixel.
 *   map + map_offsets[b] (bytes)     h_b × w_b int16, row-major: the LOWEST drawn i with P_i[y,x] = 1, or -1.  Rows leave the
 *                                    detection layer in descending score, so the most confident instance owns a contested pixel.
 *                                    This departs from the reference on purpose: DetectionRenderer.swift:26-41 paints row after row,
 *                                    so there the LAST — least confident — row covers the others.
 *   visible_areas (batch, rows)      uint32, may be NULL: the number of pixels of image b whose map value is i.
 *   detections_src                   written exactly as mrcnn_paste_masks_source writes it.
 * rows <= 32767 (the map is int16).
 *
 * mrcnn_render_detections_source — DetectionRenderer.swift:26-88: the detections drawn over the source images, RGB8 interleaved.
 *   images[b]                        the source image, as given to mrcnn_maskrcnn_predict_images (read, never written)
 *   out_rgb + out_offsets[b]         h_b × w_b × 3 bytes.  Row i has colour palette[i % 4], palette = red (255,0,0), blue (0,0,255),
 *                                    green (0,255,0), yellow (255,255,0) (DetectionRenderer.swift:53).  The stroke of row i, `stroke`
 *                                    pixels wide, is the part of OUTER that is not in INNER: OUTER = box_i grown by stroke/2 (integer
 *                                    division) on every side and clipped to the image, INNER = box_i shrunk by stroke - stroke/2 on
 *                                    every side (stroke = 3, the reference's lineWidth: one pixel outside the box, two inside); an
 *                                    empty or inverted INNER leaves the whole OUTER; stroke = 0 draws none.  Per pixel and channel c:
 *                                      under the stroke of a drawn row: the colour of the lowest such row, opaque;
 *                                      else, map[y,x] >= 0:            (src_c * (256 - alpha) + colour_c * alpha + 128) >> 8
 *                                                                      (alpha 256 = the reference's opaque fill);
 *                                      else:                           src_c.
 *   detections_src                   as above; may be NULL.
 * alpha in 0..256, stroke in 0..65534.  out_rgb must not overlap the source images.
 *
 * Conventions of both, as mrcnn_paste_masks_source: memspace holds for every data pointer (and for the rgb pointers of `images`);
 * heights, widths, the offsets and the image table are host memory.  Offsets are BYTE offsets, each a multiple of 16; the images'
 * ranges must not overlap, bytes no image covers are left untouched.  One launch per call for the whole batch, after the box mapping.
 * Errors (the message names the index of the offending image): null pointer, bad offsets -> MRCNN_ERR_INVALID; a side outside
 * 1..32767, rows > 32767, alpha or stroke out of range -> MRCNN_ERR_SHAPE; no gfx950 device -> MRCNN_ERR_HIP (no CPU fallback). */
MRCNN_API int mrcnn_instance_map_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                        const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                        float min_score, int memspace, float* detections_src, int16_t* map, const int64_t* map_offsets,
                                        uint32_t* visible_areas);
MRCNN_API int mrcnn_render_detections_source(const mrcnn_image* images, const float* detections, const float* masks, int batch, int rows,
                                             int mask_size, int model_h, int model_w, float threshold, float min_score, int alpha, int stroke,
                                             int memspace, float* detections_src, uint8_t* out_rgb, const int64_t* out_offsets);

/* Tiled prediction: large images (aerial scenes, slides, 4K/8K frames) predicted as overlapping windows at native resolution, the
 * duplicates of the overlaps removed on the GPU.  Letterboxing such an image into the model's input shrinks its objects below the
 * RPN's smallest anchors; a window is letterboxed with its OWN geometry, exactly as an image of the window's size would be.
 *
 * mrcnn_tile_plan — host only, no GPU.  Per axis with length L, tile T and overlap O (0 <= O < T): L <= T gives the one window
 *   [0, L); otherwise the stride is s = T - O, there are ceil((L - T) / s) + 1 windows and window k starts at min(k*s, L - T): every
 *   window is exactly T long, the last one is shifted inward instead of being cut.  Tiles are listed row-major (y outer, x inner) with
 *   .image = image.  *count is always the number needed; out = NULL (capacity 0) is the size query; a capacity that is too small, a bad
 *   overlap or a side outside 1..32767 -> MRCNN_ERR_SHAPE.
 *
 * mrcnn_maskrcnn_predict_tiles — record t (detections (n_tiles, maxDetections, 6), masks (n_tiles, maxDetections, S, S)) equals
 *   mrcnn_maskrcnn_predict_images on a contiguous copy of window t alone, bit for bit, in every compute mode.  Any window size is
 *   allowed.  n_tiles may exceed max_batch: the call runs ceil(n_tiles / max_batch) predicts of up to max_batch tiles each (range
 *   recovery of the split modes works per predict).  Every source image is copied to the device ONCE (MRCNN_DEVICE: read in place);
 *   the windows are never materialised on either side — the pre-processing addresses a window through its image's row pitch.
 *   memspace holds for the rgb pointers and both outputs; the two tables are host memory.  Synchronous; never replayed from a captured
 *   graph.  Errors (the message names the tile): null pointer -> MRCNN_ERR_INVALID; n_tiles < 1, tile.image outside 0..n_images-1, an
 *   empty window or one not inside its image -> MRCNN_ERR_SHAPE.
 *
 * mrcnn_merge_tiles (device) / mrcnn_merge_tiles_host (the definition: sequential plain C++, no GPU) — the records of predict_tiles
 *   in the frame of the images the windows were cut from, cross-tile duplicates dropped.  The device entry equals the host entry bit
 *   for bit.  Candidate k = t*rows + i is row i of tile t:
 *     box      its pixel box (y1, x1, y2, x2) in the tile (what mrcnn_paste_masks_source derives for an image of the tile's size)
 *              plus (y0, x0, y0, x0) of the tile;
 *     plane    P_k, h_img x w_img: zero outside the window, inside it the plane mrcnn_paste_masks_source pastes for the tile alone;
 *     row      (y1 / max(h-1,1), x1 / max(w-1,1), (y2-1) / max(h-1,1), (x2-1) / max(w-1,1), class, score) of the full-frame box,
 *              each quotient computed in double and rounded to float once.  For sides <= 32767 the rounding error is at most
 *              32767 * 2^-24 (0.002 pixel), so denorm_boxes of the row returns the full-frame pixel box again: handed these rows
 *              (as `detections`, with heights/widths = model_h/model_w = the image's size, i.e. an identity letterbox, one image
 *              at a time) mrcnn_paste_masks_source and the renderers give P_k.
 *   A candidate is ELIGIBLE if its score is > 0 and its box is not empty.  Per image the eligible candidates are walked by score
 *   descending, ties by k ascending; candidate c is DROPPED if an earlier KEPT candidate q of the same image has the same class id,
 *   tile(q) != tile(c) and m(q, c) >= match_threshold, where inter = |P_q & P_c| (an exact integer), a = the planes' areas and
 *     MRCNN_MATCH_IOU: m = inter / (a_q + a_c - inter)        MRCNN_MATCH_IOS: m = inter / min(a_q, a_c)
 *   as IEEE double divisions of those integers, 0/0 = 0.  A dropped candidate suppresses nothing; rows of one tile are never compared
 *   (the detection layer's own NMS ran there).  This entry only drops candidates: an object is recovered whole by it only if some
 *   window contains it whole; IoS is the metric that removes a cut copy of an object in favour of its whole copy.  The cut parts of
 *   an object that no window holds whole are united into one mask by mrcnn_unite_tiles (below).
 *   Outputs, per image the first max_out kept candidates in that order:
 *     detections_src (n_images, max_out, 6)   the rows above, zero-padded
 *     source (n_images, max_out)              the candidate index k, -1 for padding
 *     n_kept (n_images)                       the number kept BEFORE the cap (n_kept > max_out: the output was truncated)
 *     counts / run_offsets (n_images*max_out + 1) / areas / bboxes_xywh   the kept planes as COCO RLE in mrcnn_masks_rle_source's
 *                                             layout and capacity protocol (padding = the single run [h*w]; capacity 0 with counts
 *                                             NULL = the size query, everything but counts is written; too small -> MRCNN_ERR_SHAPE
 *                                             with the size needed in the message); areas / bboxes_xywh may be NULL.
 *   memspace holds for detections, masks and every output; the tile table and the sizes are host arrays.  match_threshold > 0.
 *   An image may have at most MRCNN_TILES_MAX_CANDIDATES candidates (its tiles x rows: 81 tiles of 100 rows), beyond ->
 *   MRCNN_ERR_SHAPE.  Argument errors as predict_tiles'; unknown metric, match_threshold <= 0 -> MRCNN_ERR_INVALID; rows, n_images or
 *   max_out < 1 -> MRCNN_ERR_SHAPE.  Every argument error is answered before a device is looked for.
 *
 * mrcnn_unite_tiles (device) / mrcnn_unite_tiles_host (the definition: sequential plain C++, no GPU) — the same records with the cut
 *   parts of an object, and its duplicates, united into ONE mask.  The device entry equals the host entry bit for bit.  Candidates,
 *   eligibility, boxes, planes, rows and the per-image order (score descending, ties by k ascending) are mrcnn_merge_tiles'.
 *   LINK: two eligible candidates q, c of one image are linked if they have the same class id, tile(q) != tile(c), the two windows
 *   share a non-empty rectangle R and m_R(q, c) >= link_threshold, where inter = |P_q & P_c| (it lies inside R), a_qR = |P_q & R|,
 *   a_cR = |P_c & R| and
 *     MRCNN_MATCH_IOU: m_R = inter / (a_qR + a_cR - inter)    MRCNN_MATCH_IOS: m_R = inter / min(a_qR, a_cR)
 *   as IEEE double divisions of those integers, 0/0 = 0: the agreement of the two masks where both windows could see the object.  It
 *   is 1 where a cut part meets its continuation, where a cut copy meets the whole copy and where two whole copies lie inside the
 *   overlap, so one rule covers fragments and duplicates.  Rows of one tile are never linked.
 *   COMPONENTS: the connected components of the link graph (transitive: an object crossing three windows in a row is one component
 *   even if the first and the last window share nothing; a wrongly chained component is not split — link_threshold is the control).
 *   A component's REPRESENTATIVE is its member earliest in the order; components are listed by their representative's place.
 *   Outputs, per image the first max_out components, as mrcnn_merge_tiles' with
 *     plane (counts / areas / bboxes_xywh)    the OR of the members' planes (a run one member ends exactly where another begins is
 *                                             one run; positions are linear, also across a column boundary); bboxes_xywh is the
 *                                             tight box of the set pixels
 *     detections_src                          the row, computed as above, of the hull of the members' full-frame boxes (min y1, x1,
 *                                             max y2, x2); class and score are the representative's
 *     source                                  the representative's k
 *     n_kept                                  the number of components before the cap
 *     n_parts (n_images, max_out)             the number of members, 0 for padding; may be NULL
 *     group (n_tiles, rows)                   per candidate the index of its component within its image in the output order (>=
 *                                             max_out where the output was truncated), -1 if not eligible; may be NULL
 *   A component of one member is, bit for bit, what mrcnn_merge_tiles outputs for that candidate when kept.  link_threshold > 0;
 *   limits, errors and the capacity protocol are mrcnn_merge_tiles'.  A united mask is no longer a pasted S x S mask:
 *   mrcnn_rle_decode, mrcnn_instance_map_rle and mrcnn_render_detections_rle (below) draw it from its RLE.  Objects are not united
 *   across images.
 * examples/maskrcnn_predict_tiled.c is the whole flow as a C99 host. */
typedef struct { int32_t image, y0, x0, height, width; } mrcnn_tile;   /* a window of images[image] */
enum { MRCNN_MATCH_IOU = 0, MRCNN_MATCH_IOS = 1 };
#define MRCNN_TILES_MAX_CANDIDATES 8192
MRCNN_API int mrcnn_tile_plan(int height, int width, int tile_h, int tile_w, int overlap_y, int overlap_x, int image, mrcnn_tile* out,
                              int capacity, int* count);
MRCNN_API int mrcnn_maskrcnn_predict_tiles(mrcnn_model* model, const mrcnn_image* images, int n_images, const mrcnn_tile* tiles,
                                           int n_tiles, int memspace, float* detections, float* masks);
MRCNN_API int mrcnn_merge_tiles(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold,
                                int metric, double match_threshold, int max_out, int memspace, float* detections_src, int32_t* source,
                                int32_t* n_kept, uint32_t* counts, int64_t capacity, int64_t* run_offsets, uint32_t* areas,
                                int32_t* bboxes_xywh);
MRCNN_API int mrcnn_merge_tiles_host(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows,
                                     int mask_size, const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w,
                                     float threshold, int metric, double match_threshold, int max_out, float* detections_src,
                                     int32_t* source, int32_t* n_kept, uint32_t* counts, int64_t capacity, int64_t* run_offsets,
                                     uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_unite_tiles(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold,
                                int metric, double link_threshold, int max_out, int memspace, float* detections_src, int32_t* source,
                                int32_t* n_kept, int32_t* n_parts, int32_t* group, uint32_t* counts, int64_t capacity,
                                int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_unite_tiles_host(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows,
                                     int mask_size, const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w,
                                     float threshold, int metric, double link_threshold, int max_out, float* detections_src,
                                     int32_t* source, int32_t* n_kept, int32_t* n_parts, int32_t* group, uint32_t* counts,
                                     int64_t capacity, int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh);

/* Drawing run-length masks: dense planes, the instance-id map and the rendered overlay from an RLE SET in the layout mrcnn_masks_rle_source,
 * mrcnn_merge_tiles, mrcnn_unite_tiles and mrcnn_rle_from_polygons_batch write: counts (uint32, column-major runs, position p = x*h + y,
 * counts[0] = the leading zeros), run_offsets (int64, n_images*slots + 1 entries); RLE k = b*slots + i belongs to image b, which is
 * heights[b] x widths[b].  Zero-length runs are legal anywhere.  An RLE whose runs do not sum to exactly h_b*w_b makes the call return
 * MRCNN_ERR_SHAPE (the message names k) with nothing written to the outputs.  P_k is the h_b x w_b {0,1} plane RLE k encodes.
 *   mrcnn_rle_decode             out + out_offsets[b] + i*h_b*w_b = P_k, row-major uint8 {0,1}: the layout mrcnn_paste_masks_source writes,
 *                                so mrcnn_png_encode_batch(MRCNN_PNG_GREY8) takes it unchanged.  A subset of one image: run_offsets + first
 *                                with a smaller slots.
 *   mrcnn_instance_map_rle       box_i = the pixel box of row i of detections_src (n_images, slots, 6) in its image's own frame: round-half-
 *                                even of y*(h_b-1), + 1 on the exclusive far edge.  Row i is DRAWN if score > min_score, score > 0 and
 *                                box_i is not empty.  map[y,x] (int16) = the lowest drawn i with P_k[y,x] = 1, else -1;
 *                                visible_areas[b,i] (may be NULL) = the pixels i owns.  slots <= 32767.  The box only decides whether a row
 *                                is drawn: set pixels outside it count (a united mask's hull box or a user's box need not be tight).
 *   mrcnn_render_detections_rle  images[b] drawn over: stroke ring, blend, palette i % 4 and the ranges of alpha and stroke in the words of
 *                                mrcnn_render_detections_source, with P_k in place of the pasted plane.
 * Conventions are mrcnn_instance_map_source's: memspace holds for every data pointer (run_offsets and the images' rgb pointers too); sizes,
 * offsets and the image table are host arrays; offsets are byte offsets, multiples of 16, the images' ranges must not overlap and bytes no
 * image covers are left untouched.  Errors: null pointer, bad output offsets -> MRCNN_ERR_INVALID; a side outside 1..32767, slots > 32767
 * (map, render), alpha or stroke out of range, decreasing run_offsets -> MRCNN_ERR_SHAPE; argument errors are answered before a device is
 * looked for; no gfx950 device -> MRCNN_ERR_HIP from the device entries (no CPU fallback).  The _host entries are the definition —
 * sequential plain C++, no GPU, host pointers — which the device entries equal byte for byte.  examples/maskrcnn_render_tiled.c. */
MRCNN_API int mrcnn_rle_decode(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                               const int32_t* widths, int memspace, uint8_t* out, const int64_t* out_offsets);
MRCNN_API int mrcnn_rle_decode_host(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                    const int32_t* widths, uint8_t* out, const int64_t* out_offsets);
MRCNN_API int mrcnn_instance_map_rle(const float* detections_src, const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots,
                                     const int32_t* heights, const int32_t* widths, float min_score, int memspace, int16_t* map,
                                     const int64_t* map_offsets, uint32_t* visible_areas);
MRCNN_API int mrcnn_instance_map_rle_host(const float* detections_src, const uint32_t* counts, const int64_t* run_offsets, int n_images,
                                          int slots, const int32_t* heights, const int32_t* widths, float min_score, int16_t* map,
                                          const int64_t* map_offsets, uint32_t* visible_areas);
MRCNN_API int mrcnn_render_detections_rle(const mrcnn_image* images, const float* detections_src, const uint32_t* counts,
                                          const int64_t* run_offsets, int n_images, int slots, float min_score, int alpha, int stroke,
                                          int memspace, uint8_t* out_rgb, const int64_t* out_offsets);
MRCNN_API int mrcnn_render_detections_rle_host(const mrcnn_image* images, const float* detections_src, const uint32_t* counts,
                                               const int64_t* run_offsets, int n_images, int slots, float min_score, int alpha, int stroke,
                                               uint8_t* out_rgb, const int64_t* out_offsets);

/* Host only, no GPU: COCO's compressed string of one RLE (pycocotools rleToString / rleFrString), not NUL-terminated.  *length / *n is
 * always the size needed; with out / counts = NULL the call only measures, a buffer that is too small gives MRCNN_ERR_SHAPE. */
MRCNN_API int mrcnn_rle_to_string(const uint32_t* counts, int64_t n, char* out, int64_t capacity, int64_t* length);
MRCNN_API int mrcnn_rle_from_string(const char* s, int64_t length, uint32_t* counts, int64_t capacity, int64_t* n);
/* 28×28 mask → 8-bit: UInt8(255 - v/2*255) (Detection.swift:83-85). */
MRCNN_API int mrcnn_mask_to_u8(const float* mask, int64_t n, uint8_t* out);
/* The same on Double input — the type Core ML hands maskFromFeatureValue (Detection.swift:77); for hosts that widen the fp32
 * mask of mrcnn_maskrcnn_predict first the result is identical (float → double is exact). */
MRCNN_API int mrcnn_mask_to_u8_f64(const double* mask, int64_t n, uint8_t* out);

/* ---------------------------------------------------------------------------------------------
 * COCO scoring — the second half of `maskrcnn evaluate` (Sources/maskrcnn/Python/COCOEval/task.py:93-98,
 * coco_dataset.evaluate_results: COCOeval's evaluate step).  The IoU of every detection with every ground truth of its image and the
 * greedy matching per (image, category, area range, IoU threshold) run on the GPU, and so does accumulate (mrcnn_coco_accumulate);
 * summarize — twelve means — is left to the host (coco_eval.py).  RLE sets are in the layout of mrcnn_masks_rle_source: RLE k = counts[run_offsets[k] .. run_offsets[k+1]),
 * uint32 run lengths, column-major, counts[0] = leading zeros; n + 1 offsets, non-decreasing, run_offsets[0] >= 0.
 *
 * mrcnn_iou_group — one image: detections [d0, d1) of the detection set against ground truths [g0, g1) of the ground-truth set; the
 * (d1-d0) x (g1-g0) results, row-major (detection-major), start at out_offset of the outputs, which hold n_pairs entries; blocks of
 * different groups must not overlap, entries no block covers are left untouched.
 *
 * mrcnn_rle_iou: inter = the intersection in pixels (exact), iou = inter / (area_d + area_g - inter) as IEEE double division of those
 * integers; for a ground truth with g_iscrowd != 0: inter / area_d (COCO's crowd rule); 0 / 0 = 0.  A pair whose two RLEs do not sum to
 * the same number of pixels makes the call fail with MRCNN_ERR_SHAPE (the message names the pair) before anything is written.
 * memspace holds for the counts, the run offsets, inter and iou (with MRCNN_DEVICE the buffers mrcnn_masks_rle_source wrote are read in
 * place); g_iscrowd (n_g, may be NULL = none) and groups are host arrays.  inter / iou may be NULL.
 * mrcnn_box_iou_xywh: the same for boxes (x, y, w, h as double): iw = min(xd+wd, xg+wg) - max(xd, xg), ih likewise, 0 unless both are
 * positive, else iw*ih / (wd*hd + wg*hg - iw*ih), crowd: / (wd*hd).  memspace holds for the boxes and iou.
 * --------------------------------------------------------------------------------------------- */
typedef struct { int64_t d0, d1, g0, g1, out_offset; } mrcnn_iou_group;
MRCNN_API int mrcnn_rle_iou(const uint32_t* d_counts, const int64_t* d_run_offsets, int64_t n_d, const uint32_t* g_counts,
                            const int64_t* g_run_offsets, int64_t n_g, const uint8_t* g_iscrowd, const mrcnn_iou_group* groups, int n_groups,
                            int memspace, uint32_t* inter, double* iou, int64_t n_pairs);
MRCNN_API int mrcnn_box_iou_xywh(const double* d_boxes, int64_t n_d, const double* g_boxes, int64_t n_g, const uint8_t* g_iscrowd,
                                 const mrcnn_iou_group* groups, int n_groups, int memspace, double* iou, int64_t n_pairs);
/* COCOeval.evaluateImg for many (image, category) groups at once.  iou (n_iou doubles, memspace) holds the images' IoU blocks as the two
 * calls above wrote them.  Group k: its image's block starts at iou_offset and has iou_stride columns (the image's ground truths);
 * its detections are entries [dt0, dt1) of the flat lists dt_idx (row of the block) / dt_area, ALREADY sorted by score descending
 * (stable) and cut to maxDet; its ground truths entries [gt0, gt1) of gt_idx (column of the block) / gt_area / gt_iscrowd in annotation
 * order.  The groups tile the flat lists: dt0 of group 0 is 0, dt0 of group k+1 = dt1 of group k, the last dt1 = n_dt; likewise gt.
 * For every area range a (area_ranges[2a] <= area <= area_ranges[2a+1] is inside) and threshold t:
 *   a ground truth is IGNORED when it is a crowd or its area is outside the range; COCOeval's order "non-ignored first, stable" is taken
 *   inside the kernel (it depends on a); each detection in turn takes, among the ground truths with iou >= min(t, 1 - 1e-10) that are
 *   not yet taken (a crowd can be taken again), the non-ignored one of highest IoU — the later of equals — and only if there is none
 *   the ignored one of highest IoU; a matched detection inherits the ignore flag, an unmatched one is ignored when its own area is
 *   outside the range.  "Taken" is tested as such (pycocotools tests the annotation id for > 0 instead).
 * Outputs (memspace; any may be NULL), with A = n_ranges, T = n_thresholds, nd = dt1-dt0, ng = gt1-gt0 of the group:
 *   dt_match [A*T*dt0 + (a*T + t)*nd + i]  the position in the group's ground-truth list (0..ng-1) detection i took, or -1
 *   dt_ignore[the same index]              1 / 0
 *   gt_match [A*T*gt0 + (a*T + t)*ng + j]  the position in the group's detection list that took ground truth j (the last, for a crowd), or -1
 * All tables but iou are host arrays.  Inconsistent tables (ranges out of order, an index outside its block, a block outside iou) give
 * MRCNN_ERR_SHAPE. */
typedef struct { int64_t iou_offset; int32_t iou_stride, dt0, dt1, gt0, gt1, reserved; } mrcnn_match_group;
MRCNN_API int mrcnn_coco_match(const double* iou, int64_t n_iou, int memspace, const mrcnn_match_group* groups, int n_groups,
                               const int32_t* dt_idx, const double* dt_area, int64_t n_dt, const int32_t* gt_idx, const double* gt_area,
                               const uint8_t* gt_iscrowd, int64_t n_gt, const double* area_ranges, int n_ranges,
                               const double* iou_thresholds, int n_thresholds, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match);
/* COCOeval.accumulate on the GPU: the precision / recall tables from the matching's flags.  coco_eval.accumulate (numpy) is the
 * definition; the two outputs are what it returns, bit for bit.
 * Inputs.  The detection entries are ONE flat list of n_dt entries, category-major; inside a category the images in image order; inside an
 * image the entries in descending score — the order in which accumulate concatenates its per-image records.  Category k owns the
 * entries [cat_offsets[k], cat_offsets[k+1]) (n_cats + 1 offsets, cat_offsets[0] = 0, non-decreasing, cat_offsets[n_cats] = n_dt).
 *   scores[i]                      the score of entry i
 *   ranks[i]                       the position of entry i in the list of its own (image, category): the entry TAKES PART under
 *                                  max_dets[m] iff ranks[i] < max_dets[m] (accumulate's [:maxDet] slices)
 *   dt_matched[(a*T + t)*n_dt + i] and dt_ignore[the same index]: 0 or 1, A = n_ranges, T = n_thresholds
 *   npig[k*A + a]                  the non-ignored ground truths of category k in area range a, over all images
 * memspace holds for scores, ranks, dt_matched, dt_ignore, precision and recall; cat_offsets, npig, max_dets (n_max_dets = M) and rec_thrs
 * (n_rec = R, non-decreasing) are host arrays.
 * Outputs, row-major doubles, every entry overwritten: precision (T, R, K, A, M), recall (T, K, A, M), K = n_cats.  Per (k, a, m):
 *   the entries of category k that take part, ordered as np.argsort(-scores, kind="mergesort") orders them: descending and stable, -0.0
 *   and 0.0 equal, a NaN after every number (the order under a smaller max_dets is a subsequence of the order under a larger one);
 *   per t: tp = cumsum(matched & !ignore), fp = cumsum(!matched & !ignore), counted as integers and converted to double;
 *   rc = tp / npig; pr = tp / ((fp + tp) + 2.220446049250313e-16), in exactly that association, both IEEE double divisions;
 *   pr is replaced by its maximum over the entries from it to the end; precision[t, r] = pr[the first i with rc[i] >= rec_thrs[r]], 0
 *   where there is none; recall[t] = rc[last], 0 when no entry takes part.
 *   npig == 0: the whole (k, a, m) cell is -1 in both outputs — a category without any record is this case.
 * A category is sorted in chunks of MRCNN_COCO_ACC_CHUNK entries in LDS which are then merged pairwise in global memory, and scanned
 * in chunks of the same size with a carry; there is no limit on the size of a category (n_dt < 2^31), and the number of launches grows
 * with the logarithm of the largest category, not with n_cats.  The flag planes are permuted into sorted order once.
 * Errors, all before the device is touched: a null pointer (scores, ranks, dt_matched, dt_ignore only when n_dt > 0; npig, precision,
 * recall only when n_cats > 0), negative n_dt / n_cats, an unknown memspace, cat_offsets that decrease, do not start at 0 or do not end at
 * n_dt, a negative npig -> MRCNN_ERR_INVALID; n_ranges, n_thresholds, n_max_dets or n_rec below 1, rec_thrs that decrease (or hold a NaN),
 * tables too large for one call (n_dt >= 2^31, K*A*M*T >= 2^31) -> MRCNN_ERR_SHAPE.  No gfx950 device -> MRCNN_ERR_HIP (no CPU fallback).
 * n_dt = 0 and n_cats = 0 are valid. */
#define MRCNN_COCO_ACC_CHUNK 1024
MRCNN_API int mrcnn_coco_accumulate(const double* scores, const int32_t* ranks, const uint8_t* dt_matched, const uint8_t* dt_ignore,
                                    int64_t n_dt, const int64_t* cat_offsets, int n_cats, const int64_t* npig, int n_ranges, int n_thresholds,
                                    const int32_t* max_dets, int n_max_dets, const double* rec_thrs, int n_rec, int memspace, double* precision,
                                    double* recall);
/* Host only, no GPU: the union of n_polys COCO polygons (polygon p = the points xy[2*poly_offsets[p]] .. xy[2*poly_offsets[p+1]), x
 * then y, in pixels) on an h x w plane as ONE RLE, by COCO's published procedure (pycocotools rleFrPoly): vertices scaled by 5 and
 * rounded, the edges walked on that fine grid, the crossings of pixel-column centres reduced to column-major run boundaries (clipped
 * to the plane), the polygons of one annotation united.  *n is always the number of runs; counts = NULL with capacity = 0 only
 * measures, a buffer that is too small gives MRCNN_ERR_SHAPE.  Polygons partly or wholly outside the plane are clipped; a polygon of fewer than 3 points
 * or of no area still gives a valid RLE (its crossings cancel in pairs). */
MRCNN_API int mrcnn_rle_from_polygons(const double* xy, const int64_t* poly_offsets, int n_polys, int h, int w, uint32_t* counts,
                                      int64_t capacity, int64_t* n);
/* The same for a whole annotation file in one call, on the GPU.  xy / poly_offsets as above (all points; polygon p = the points
 * [poly_offsets[p], poly_offsets[p+1])); annotation k = the polygons [ann_offsets[k], ann_offsets[k+1]) on the heights[k] x widths[k]
 * plane of its image.  RLE k is, word for word, what mrcnn_rle_from_polygons returns for annotation k's polygons on that plane — that
 * function is the definition; an annotation without a polygon is the single run [h*w].  The result is an RLE set in the layout and
 * with the capacity protocol of mrcnn_masks_rle_source, ready for mrcnn_rle_iou:
 *   counts + run_offsets[k] .. counts + run_offsets[k+1]   the run lengths of annotation k (all annotations back to back)
 *   run_offsets (n_anns + 1), areas (n_anns: the set pixels = the sum of the odd runs) and bboxes_xywh (n_anns*4: the tight box x, y, w,
 *   h of the set pixels, 0,0,0,0 for none) are ALWAYS written; areas / bboxes_xywh may be NULL.
 * If run_offsets[n_anns] > capacity the call returns MRCNN_ERR_SHAPE, the message names the capacity needed and counts is not written
 * (capacity = 0 with counts = NULL is the size query).  memspace holds for counts, run_offsets, areas and bboxes_xywh; xy, poly_offsets,
 * ann_offsets, heights and widths are host arrays.  With MRCNN_HOST only the used part of counts is copied.
 * An annotation crossing at most MRCNN_POLY_LDS_TOGGLES pixel-column centres with its outlines is sorted in LDS, one with more in global
 * memory; there is no size limit beyond that of mrcnn_rle_from_polygons, and the number of launches does not depend on n_anns.
 * Errors (the message names the annotation, and the polygon inside it): null pointer, decreasing offsets -> MRCNN_ERR_INVALID; a side
 * outside 1..32767 -> MRCNN_ERR_SHAPE; a coordinate that is not finite or has |c| >= 1e6 -> MRCNN_ERR_INVALID; all of these before the
 * device is touched.  No gfx950 device -> MRCNN_ERR_HIP (no CPU fallback). */
#define MRCNN_POLY_LDS_TOGGLES 4096
MRCNN_API int mrcnn_rle_from_polygons_batch(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, int64_t n_anns,
                                            const int32_t* heights, const int32_t* widths, int memspace, uint32_t* counts, int64_t capacity,
                                            int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh);

/* Polygons out: the boundary of every mask of an RLE SET as closed rings of pixel corners, traced from the runs — no plane is decoded.
 * The input is the set of the drawing entries above (counts, run_offsets, n_images, slots, heights, widths): RLE k = b*slots + i lies on
 * the h_b x w_b plane P_k of image b; zero-length runs are legal anywhere and a run of ones that crosses a column end is two vertical
 * intervals.
 * Geometry.  Pixel (x, y) is the unit square [x, x+1] x [y, y+1], x to the right and y down.  A vertex (X, Y) is a pixel corner,
 *   0 <= X <= w, 0 <= Y <= h.  The boundary of P_k is the set of unit edges between a set pixel and an unset pixel or the outside of
 *   the plane, each directed so that the set pixel lies on its right as seen on screen: the top edge of a set pixel runs +x, its right
 *   edge +y, its bottom edge -x, its left edge -y.  Where four boundary edges meet — two set pixels touch only diagonally — the walk
 *   turns right: set pixels are 4-connected, unset pixels 8-connected, every directed edge has exactly one successor, and the edges fall
 *   into closed rings.
 * A ring keeps only its corners (collinear vertices are dropped): an even number of vertices, at least 4, horizontal and vertical
 *   pieces in turn.  It may pass twice through a vertex, only at such a diagonal contact.  It starts at its smallest vertex, ordered by
 *   x and then y, and goes on in walking direction; nothing of a ring lies left of that vertex, so the ring visits it once and no two
 *   rings of a plane start at the same vertex.  The rings of one RLE are ordered by their start vertex, x then y.  A ring's signed area
 *   is (1/2) * sum(x_i*y_{i+1} - x_{i+1}*y_i): positive for an outline, which runs clockwise on screen, negative for a hole; the areas
 *   of an RLE's rings sum to its set pixels.  An empty mask has no rings.
 * Outputs.
 *   rle_rings (n + 1, n = n_images*slots)   the rings of RLE k are [rle_rings[k], rle_rings[k+1]); ALWAYS written
 *   *n_rings, *n_vertices (host)            the totals; ALWAYS written
 *   ring_offsets (ring_capacity + 1)        ring r owns the vertices [ring_offsets[r], ring_offsets[r+1]); n_rings + 1 entries are written
 *   ring_areas (ring_capacity, may be NULL) the signed areas
 *   xy (2 * vertex_capacity, int32)         x then y per vertex, all rings back to back
 * The two capacities follow the protocol of mrcnn_masks_rle_source: if n_rings > ring_capacity or n_vertices > vertex_capacity the
 * call returns MRCNN_ERR_SHAPE, the message names both sizes needed and none of ring_offsets, ring_areas and xy is written (both
 * capacities 0 with NULL buffers is the size query).  memspace holds for counts, run_offsets, rle_rings, ring_offsets, ring_areas and
 * xy; heights, widths, n_rings and n_vertices are host memory.
 * mrcnn_rle_to_polygons_host is the definition: sequential plain C++, no GPU, host pointers; it decodes each plane and walks its edges
 * one by one.  mrcnn_rle_to_polygons equals it bit for bit in every array.  It finds the corners of a vertex column by merging the runs
 * of the two pixel columns beside it, pairs them along columns and rows, and orders the cycles of that permutation by pointer
 * jumping; an RLE of at most MRCNN_POLYGON_LDS_CORNERS corners is sorted and ranked by one workgroup in LDS, a larger one in global
 * memory.  The number of launches grows with the square of the logarithm of the largest RLE's corners, never with the number of RLEs;
 * the host reads back one summary (is every RLE right, how many corners) before anything is traced and the number of rings after.
 * Errors are mrcnn_rle_decode's: null pointer, negative capacity -> MRCNN_ERR_INVALID; a side outside 1..32767, decreasing
 * run_offsets -> MRCNN_ERR_SHAPE; an RLE whose runs do not sum to h_b*w_b -> MRCNN_ERR_SHAPE, the message names k and nothing is
 * written; all of these before a device is looked for, except the sums of a set in device memory.  No gfx950 device -> MRCNN_ERR_HIP
 * from the device entry (no CPU fallback).
 * Simplification (Douglas-Peucker) is the next entry's, mrcnn_polygons_simplify, which takes ring_offsets and xy as they are written
 * here; nesting the rings into outlines and their holes is mrcnn_polygons_nest's, below: here a hole is a ring of negative area and
 * nothing more.  Not here: smoothing and sub-pixel contours from the 28x28 probabilities.  examples/maskrcnn_polygons.c. */
#define MRCNN_POLYGON_LDS_CORNERS 1024
MRCNN_API int mrcnn_rle_to_polygons(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                    const int32_t* widths, int memspace, int64_t* rle_rings, int64_t* n_rings, int64_t* n_vertices,
                                    int64_t* ring_offsets, int64_t* ring_areas, int64_t ring_capacity, int32_t* xy, int64_t vertex_capacity);
MRCNN_API int mrcnn_rle_to_polygons_host(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                         const int32_t* widths, int64_t* rle_rings, int64_t* n_rings, int64_t* n_vertices,
                                         int64_t* ring_offsets, int64_t* ring_areas, int64_t ring_capacity, int32_t* xy, int64_t vertex_capacity);

/* Polygon rings simplified on the GPU: Douglas-Peucker with a tolerance in pixels, exact in integers.  The input is rings in the layout
 * mrcnn_rle_to_polygons writes — ring r = the vertices [ring_offsets[r], ring_offsets[r+1]) of xy (int32 x then y) — but any integer
 * rings are legal, not only traced ones: every coordinate in 0..32767, every ring under 2^31 vertices, offsets that start at 0 or above
 * and do not decrease.  A ring is closed: its last vertex is joined to its first.
 * Tolerance.  A double, finite, 0 <= tolerance <= 65535.  It becomes one integer once, on the host: E = floor(tolerance * tolerance *
 *   65536) (the products rounded as doubles).  Nothing after that touches floating point.
 * The ring rule.  A ring of m vertices v_0 .. v_{m-1}: if m <= 2 it is copied as it is.  Otherwise it has two anchors, which are kept:
 *   v_0, and v_f, the vertex of largest squared Euclidean distance from v_0, the smallest index on a tie.  The two open chains
 *   v_0 .. v_f and v_f .. v_m (v_m is v_0 again) are simplified independently by the chain rule.
 * The chain rule.  A chain with end vertices a and b and at least one vertex strictly between them: every such vertex p has the
 *   distance c(p) = |(b - a) x (p - a)| = |(bx - ax)*(py - ay) - (by - ay)*(px - ax)|, or, when a and b have equal coordinates (a ring
 *   may pass twice through a vertex), c(p) = |p - a|^2.  The chosen vertex has the largest c; a tie goes to the smallest position along
 *   the chain.  It is kept iff c*c*65536 > E*|b - a|^2 (an exact comparison of up to 79 bits), for equal a and b iff c*65536 > E: iff it
 *   lies farther than the tolerance from the chord.  If it is kept, the chains a .. p and p .. b are handled by the same rule; if not,
 *   every vertex strictly between a and b is dropped.
 * What follows: the output ring is a subsequence of the input ring and starts at the same vertex; rings stay in their order, one for
 *   one, so rle_rings of the tracer still indexes them.  Tolerance 0 returns a traced ring unchanged (horizontal and vertical pieces in
 *   turn leave no vertex on a chord).  The kept sets are nested: a larger tolerance keeps a subset.  A ring may come out with 2 vertices
 *   (with 1 if all its vertices are equal).  TOPOLOGY IS NOT PRESERVED: rings may touch or cross themselves and one another afterwards.
 * Outputs.
 *   out_ring_offsets (n_rings + 1)          ring r owns the vertices [out_ring_offsets[r], out_ring_offsets[r+1]); ALWAYS written
 *   *n_vertices_out (host)                  the vertices of all simplified rings; ALWAYS written
 *   out_areas2 (n_rings, may be NULL)       TWICE the signed shoelace area of each simplified ring, sum(x_i*y_{i+1} - x_{i+1}*y_i): an
 *                                           integer where the area itself need not be one
 *   out_xy (2 * vertex_capacity, int32)     the simplified vertices, all rings back to back
 *   out_src_index (vertex_capacity, may be NULL)   per output vertex its index in the input xy: strictly increasing within a ring
 * Capacity, the protocol of mrcnn_rle_to_polygons: if *n_vertices_out > vertex_capacity the call returns MRCNN_ERR_SHAPE, the message
 * names the size needed and none of out_xy, out_areas2 and out_src_index is written (capacity 0 with NULL buffers is the size query;
 * the input's vertex count always suffices).  memspace holds for ring_offsets, xy and the four output arrays; n_vertices_out is host memory.
 * mrcnn_polygons_simplify_host is the definition: sequential plain C++ with an explicit stack, no GPU, host pointers.
 * mrcnn_polygons_simplify equals it bit for bit in every array.  The chains of a ring are independent, so it runs them level by level:
 * one workgroup owns a ring, every vertex knows its chain, a 64-bit maximum per chain picks the vertex, and the loop ends when no chain
 * is left — in LDS for a ring of at most MRCNN_SIMPLIFY_LDS_VERTICES vertices, in global scratch above.  Three launches and a prefix
 * sum, whatever the number of rings and the depth of the recursion; the host reads back one summary (are the rings legal, how large is
 * the largest) before anything is written and the size needed after the count.
 * Errors: null pointer (out_xy only with a capacity, xy only with rings), negative n_rings or capacity, a tolerance that is NaN or outside
 * 0..65535, unknown memspace -> MRCNN_ERR_INVALID; offsets that are negative, decrease or span 2^31 vertices, or a coordinate outside
 * 0..32767 -> MRCNN_ERR_SHAPE, the message names the ring and nothing is written; all of these before a device is looked for, except
 * the contents of rings in device memory.  No gfx950 device -> MRCNN_ERR_HIP from the device entry (no CPU fallback).
 * Not here: topology-preserving simplification, Visvalingam-Whyatt, smoothing.  examples/maskrcnn_polygons.c --tolerance. */
#define MRCNN_SIMPLIFY_LDS_VERTICES 1024
MRCNN_API int mrcnn_polygons_simplify(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance, int memspace,
                                      int64_t* out_ring_offsets, int64_t* out_areas2, int32_t* out_xy, int64_t* out_src_index,
                                      int64_t* n_vertices_out, int64_t vertex_capacity);
MRCNN_API int mrcnn_polygons_simplify_host(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance,
                                           int64_t* out_ring_offsets, int64_t* out_areas2, int32_t* out_xy, int64_t* out_src_index,
                                           int64_t* n_vertices_out, int64_t vertex_capacity);

/* Polygon rings nested on the GPU into outlines and their holes: which ring lies directly inside which, how deep, and the rings grouped
 * into polygons of one shell and its holes — what GeoJSON, WKT and GIS layers take.  The input is rings in the tracer's layout: the rings
 * of RLE k are [rle_rings[k], rle_rings[k+1]) (rle_rings has n_rles + 1 entries, starts at 0 and ends at n_rings), ring r = the vertices
 * [ring_offsets[r], ring_offsets[r+1]) of xy (int32 x then y).  Any integer rings are legal, as for mrcnn_polygons_simplify: every
 * coordinate in 0..32767, every ring closed and under 2^31 vertices, offsets that do not decrease.  The rule is total on all of them;
 * only traced rings come with the geometric guarantee.  Everything is integer arithmetic; no input array of areas is trusted.  Rings are
 * nested among the rings of their own RLE, never across RLEs; parent holds GLOBAL ring indices.
 * area2(r).  Twice the signed shoelace area of ring r, sum(x_i*y_{i+1} - x_{i+1}*y_i), 64 bits, from xy.
 * probe(r).  The point (X0 + 1/2, Y0 + 1/2), where (X0, Y0) is r's first vertex; a ring without vertices has no probe and no parent.
 *   For a traced ring the probe is the centre of a pixel that r encloses, a set pixel for an outline and an unset pixel for a hole: the
 *   ring starts at its smallest vertex and nothing of the ring lies left of its start vertex (the tracer's geometry, above), so the unit
 *   edge (X0, Y0) - (X0, Y0 + 1) is the ring's only crossing of a ray from the probe towards -x.
 * contains(q, r).  The ray from probe(r) towards -x crosses an odd number of q's edges, the closing edge included.  An edge a -> b
 *   crosses iff (ay <= Y0) != (by <= Y0) and its intersection with the line y = Y0 + 1/2 lies at x < X0 + 1/2, decided in doubled
 *   integers by the sign of (bx - ax)*(2*Y0 + 1 - 2*ay) - (by - ay)*(2*X0 + 1 - 2*ax), corrected by the sign of by - ay: no division, no
 *   floating point; 0 — the probe on the edge's line — is not a crossing.  No vertex lies on the ray's line.  For axis-parallel rings this
 *   counts the vertical edges with x <= X0 whose y-span holds Y0.  A ring of fewer than 3 vertices contains nothing.
 * parent(r).  Among the rings q != r of the same RLE with contains(q, r), those that OUTRANK r: |area2(q)| > |area2(r)|, or equal with
 *   q < r.  The parent is the one of smallest |area2|, a tie goes to the smallest index; -1 if there is none.  Outranking is a strict
 *   total order, so the result is a forest on any input; on traced rings the parent is the innermost enclosing ring.
 * depth(r).  The number of ancestors along the parent chain.  On traced rings even depth means outline (area > 0) and odd depth hole; a
 *   hole's parent is the outline of the 4-connected component around it, an outline's parent the hole it is an island of.
 * Polygons.  A ring of even depth is a shell, its children (of odd depth) are its holes.  The polygons of an RLE are ordered by their
 *   shell's ring index; inside a polygon the shell comes first, then its holes by ring index.  An island inside a hole is a polygon of
 *   its own.
 * Outputs.
 *   parent (n_rings, int64)         the global index of the ring's parent, or -1
 *   depth (n_rings, int32)
 *   rle_polys (n_rles + 1)          the polygons of RLE k are [rle_polys[k], rle_polys[k+1])
 *   poly_rings (n_rings + 1)        polygon p of the whole set owns ring_order[poly_rings[p] .. poly_rings[p+1]), shell first;
 *                                   *n_polys + 1 entries are written
 *   ring_order (n_rings)            a permutation of the rings
 *   *n_polys (host)                 n_polys <= n_rings: the buffers are sized by n_rings and there is no capacity protocol
 * memspace holds for every array argument; n_polys is host memory.  n_rings = 0 is legal: rle_polys is all zeros and *n_polys = 0.
 * Simplified rings.  mrcnn_polygons_simplify keeps the rings in their order and number, so a nesting computed on the TRACED rings
 * indexes the simplified ones, one for one: nest first, then simplify.  Nesting simplified rings themselves is legal and yields a forest,
 * but simplification does not preserve topology and the probe's guarantee is the traced rings' alone.
 * mrcnn_polygons_nest_host is the definition: sequential plain C++, no GPU, host pointers; per ring it loops over the other rings of the
 * RLE and over their edges.  mrcnn_polygons_nest equals it bit for bit in every array.  One wave per ring measures |area2|, the bounding
 * box and the owning RLE; one workgroup per target ring finds the parent, its waves striding over the candidates — one whose bounding
 * box does not hold the probe is skipped, which cannot change a parity — and their lanes over a candidate's edges; a thread per ring
 * walks to the root; two prefix sums and a rank among siblings, counted by a wave, place every ring.  Eight launches and two scans,
 * whatever the number of rings and RLEs; the host reads back one summary (are the arrays legal) before anything is written and the
 * number of polygons at the end.
 * Errors: null pointer, negative n_rles or n_rings, unknown memspace -> MRCNN_ERR_INVALID; rle_rings that does not start at 0, decreases
 * or does not end at n_rings, offsets that are negative, decrease or span 2^31 vertices, a coordinate outside 0..32767 ->
 * MRCNN_ERR_SHAPE, the message names the RLE or the ring and nothing is written; all of these before a device is looked for, except
 * the contents of arrays in device memory, which one summary answers.  No gfx950 device -> MRCNN_ERR_HIP from the device entry (no CPU
 * fallback).
 * Not here: the work is O(rings x vertices) per RLE — small for detector masks (a few rings per detection; 317 rings on the README's
 * large scene), large for a pathological plane such as a megapixel checkerboard.  The sweep that would replace the quadratic stage —
 * per probe the nearest vertical edge to its left, then pointer jumping over "sibling of" — is not built.  The depth is one thread's walk
 * to the root per ring, in one launch: on a deep chain such as concentric rings the lanes of a wave wait for the longest walk, which
 * the quadratic stage before it has outweighed already; pointer jumping in rounds is not built.  Neither are WKT, topology
 * repair of simplified rings, or nesting across RLEs.  examples/maskrcnn_polygons.c --geojson. */
MRCNN_API int mrcnn_polygons_nest(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings,
                                  int memspace, int64_t* parent, int32_t* depth, int64_t* rle_polys, int64_t* poly_rings, int64_t* ring_order,
                                  int64_t* n_polys);
MRCNN_API int mrcnn_polygons_nest_host(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings,
                                       int64_t* parent, int32_t* depth, int64_t* rle_polys, int64_t* poly_rings, int64_t* ring_order,
                                       int64_t* n_polys);

/* ---- changing run-length masks: erosion, dilation and the boundary band (csrc/api_rle_morph.hip, kernels_rle_morph.hip) --------------
 * Morphology with a square structuring element on a set of RLEs in the layout of every entry above (uint32 column-major runs, counts[0]
 * the leading zeros, int64 run_offsets): RLE in, RLE out, no dense plane.  The set is flat: RLE k is counts[run_offsets[k] ..
 * run_offsets[k+1]) and encodes a heights[k] x widths[k] plane; heights, widths and radii are HOST arrays of n (a detection set repeats
 * its image's size per slot, a ground-truth set is ragged per image).  Input RLEs may hold zero-length runs anywhere.
 * The rule (csrc/morph_rule.h).  P is the h x w {0,1} plane of an RLE, r = radii[k] >= 0; pixels outside the image are 0 for every op.
 *   MRCNN_MORPH_ERODE     E_r(P)[y,x] = 1 iff P[y',x'] = 1 for all |y'-y| <= r, |x'-x| <= r: a mask erodes from the image border too
 *   MRCNN_MORPH_DILATE    D_r(P)[y,x] = 1 iff some in-image P[y',x'] = 1 with |y'-y| <= r, |x'-x| <= r: clipped to the image
 *   MRCNN_MORPH_BOUNDARY  P AND NOT E_r(P): the inner band of width r — the band of Boundary IoU (Cheng et al., CVPR 2021), whose
 *                         published pad / iterate-3x3 / un-pad procedure with d iterations equals it at r = d
 *   r = 0: ERODE and DILATE return P, BOUNDARY the empty mask.  E_a(E_b(P)) = E_(a+b)(P) and D_a(D_b(P)) = D_(a+b)(P).
 * Outputs, exactly as mrcnn_masks_rle_source writes them: the canonical RLE of the result plane (counts[0] may be 0, no other run is,
 * runs continue across column ends, an empty plane is the single run [h*w]).
 *   out_run_offsets (n + 1)   always written
 *   areas (n), bboxes_xywh (n, 4)   optional (NULL): the set pixels and their tight box x, y, w, h (0, 0, 0, 0 for an empty mask)
 *   out_counts / capacity     written only when all runs fit: a smaller capacity -> MRCNN_ERR_SHAPE, the message names the capacity
 *                             needed (= out_run_offsets[n]) and out_counts is not written; capacity = 0 with out_counts = NULL is the
 *                             size query
 * memspace holds for counts, run_offsets and the four outputs; the outputs must not overlap the inputs.  n = 0 is legal:
 * out_run_offsets[0] = 0.
 * mrcnn_rle_morph_host is the definition: sequential plain C++, no GPU, host pointers; one RLE at a time it decodes a plane, runs the
 * two halves of the square as sliding windows over running counts, O(h*w) whatever the radius, and encodes.  mrcnn_rle_morph equals it
 * bit for bit in every output array and never builds a plane: the prefix table of the runs; one block per RLE finds the tight box of
 * its set pixels; the host reads the boxes (and the one flag that refuses a wrong total) back once and sizes a packed bit box per RLE,
 * 32 rows per word — scratch that follows the masks, not the images; one thread per box column takes the vertical half on the runs of
 * its column (an interval [a, b) becomes [a+r, b-r), or [a-r, b+r) clipped); one block per tile of a word row takes the horizontal half
 * on the words, 2r + 1 of them combined by doubling in LDS, which MRCNN_MORPH_MAX_RADIUS bounds; the encoder of mrcnn_masks_rle_source
 * runs on the bits.  Seven launches whatever n.
 * mrcnn_boundary_radius: r = max(1, round_half_even(ratio * sqrt(h*h + w*w))), evaluated in double — the published
 * int(round(dilation_ratio * img_diag)) with a floor of 1: 16 for 480x640 and 102 for 3072x4096 at ratio 0.02.
 * Errors: null pointer, unknown memspace -> MRCNN_ERR_INVALID; n < 0, a side outside 1..32767, a radius outside
 * 0..MRCNN_MORPH_MAX_RADIUS, an unknown op, run_offsets that decrease -> MRCNN_ERR_SHAPE; an RLE that does not sum to its h*w ->
 * MRCNN_ERR_SHAPE, the message starts "rle_morph:" / "rle_morph_host:" and names the lowest such k, nothing is written; a ratio that is
 * not finite or not > 0, sides outside 1..32767 -> MRCNN_ERR_SHAPE from mrcnn_boundary_radius.  Argument errors are answered before a
 * device is looked for; no gfx950 device -> MRCNN_ERR_HIP from the device entry (no CPU fallback).
 * Not here: structuring elements other than the square, grey-scale morphology, radii above the cap (compose two calls: the semigroup
 * property above). */
#define MRCNN_MORPH_ERODE 0
#define MRCNN_MORPH_DILATE 1
#define MRCNN_MORPH_BOUNDARY 2
#define MRCNN_MORPH_MAX_RADIUS 1024
MRCNN_API int mrcnn_rle_morph(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                              const int32_t* radii, int op, int memspace, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets,
                              uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_rle_morph_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                   const int32_t* radii, int op, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets,
                                   uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_boundary_radius(int h, int w, double ratio, int32_t* radius);

/* ---- cutting run-length masks into connected components (csrc/api_rle_components.hip, kernels_rle_components.hip) --------------------
 * Keep the object, drop the specks, fill the holes, or cut a mask into its parts: RLE in, measures or RLE out, no dense plane.  The set
 * is flat as mrcnn_rle_morph takes it: RLE k is counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane
 * (sides 1..32767); heights and widths are HOST arrays of n.  Zero-length runs are allowed anywhere: the result is that of the
 * canonical RLE of the same plane.
 * The rule (csrc/components_rule.h).  P is the h x w {0,1} plane of RLE k.  connectivity is 4 or 8; `of` chooses the value that is
 * labelled.  Components of ones (MRCNN_COMPONENTS_OF_ONES) use `connectivity`; components of zeros (MRCNN_COMPONENTS_OF_ZEROS) use the
 * dual, 8 where connectivity is 4 and 4 where it is 8.  At connectivity 4 the components of ones are exactly what
 * mrcnn_rle_to_polygons traces as outlines, and the components of zeros that do not touch the border exactly what it traces as holes.
 * Nothing continues outside the image.  The components of RLE k are numbered from 0 in rising order of their first pixel in
 * column-major position p = x*h + y; an empty plane (for ones) or a full one (for zeros) has none.
 * mrcnn_rle_components labels and measures — one entry per component, all components of the set back to back:
 *   comp_offsets (n + 1, int64)   always written: RLE k owns the components comp_offsets[k] .. comp_offsets[k+1]
 *   comp_areas (uint32)           the pixels of the component
 *   comp_bboxes_xywh (int32 x 4)  its tight box x, y, w, h
 *   comp_flags (uint8)            bit 0: the component holds a pixel with x == 0, x == w-1, y == 0 or y == h-1
 * The three per-component arrays are written only when comp_offsets[n] <= comp_capacity: otherwise MRCNN_ERR_SHAPE, the message names
 * the capacity needed and nothing else is written; comp_capacity = 0 with null arrays is the size query.
 * mrcnn_rle_components_select labels again and writes RLEs.  keep is one uint8 per component in the order above, in `memspace`;
 * n_comps must equal the number of components found: otherwise MRCNN_ERR_SHAPE, the message names both numbers, nothing is written.
 *   MRCNN_COMPONENTS_MERGE  n RLEs come out: a pixel of a kept component stays as it is, a pixel of a dropped component takes the other
 *                           value (of ONES: specks are cleared; of ZEROS: holes are filled), pixels of the value that was not labelled
 *                           stay.  out_parent may be NULL (else out_parent[k] = k); *out_n = n.
 *   MRCNN_COMPONENTS_SPLIT  of ONES only (else MRCNN_ERR_SHAPE): one RLE per kept component, in component order, each over its
 *                           parent's full h x w plane; out_parent[j] is the parent's k, *out_n the number kept.  out_run_offsets
 *                           holds *out_n + 1 entries: the caller gives room for n_comps + 1 (MERGE: n + 1), and for n_comps (MERGE: n)
 *                           entries of out_parent, areas and bboxes_xywh.
 * The output RLEs are canonical, exactly as mrcnn_rle_morph writes them (runs continue across column ends, an empty plane is [h*w]);
 * areas and bboxes_xywh are optional (NULL) and the out_counts / capacity protocol with its size query is mrcnn_rle_morph's:
 * out_run_offsets, out_parent, *out_n and the optional arrays are written whatever the capacity, out_counts only when all runs fit.
 * memspace holds for counts, run_offsets, keep and every output array; out_n is a host word in both memory spaces.  n = 0 is legal.
 * The _host entries are the definition: sequential plain C++, no GPU, host pointers; one RLE at a time a plane is decoded and flooded
 * from every unlabelled pixel in rising position.  The device entries equal them bit for bit in every output array and never build a
 * plane.  The nodes are PIECES: a run of the labelled value cut at the ends of its pixel columns, touching pieces of one column joined
 * first.  The pieces per run are counted and scanned, a table of (RLE, [start, end) position) is written — index order is pixel order
 * — and one thread per piece finds, with one binary search in its RLE's table and a walk, the pieces of column x + 1 that meet it:
 * rows [a, b) and [c, d) meet if a < d && c < b (4) or a <= d && c <= b (8).  Every meeting pair is united in a parent array without
 * locks: find both roots, hang the larger under the smaller with an integer compare-and-swap, retry from the value read.  The smaller
 * index always wins, so a component's root is its lowest piece whatever the order of execution and every output is deterministic; no
 * workgroup waits for another.  Root flags scanned give the rule's numbering; integer atomics give area, box and flag.  MERGE walks the
 * pieces with their keep bits — a piece starts a run unless the piece before it is kept and ends where it starts, which joins runs
 * across column ends — scans, and writes differences of positions; SPLIT first sorts the pieces by (component, piece) with a bitonic
 * network and runs the same writer per component.  The parent array lives in global memory for every RLE.  The number of launches
 * depends on neither n nor the number of components (SPLIT's sort: on the logarithm of the number of pieces).
 * Errors: null pointer, unknown memspace -> MRCNN_ERR_INVALID; n < 0, a side outside 1..32767, a connectivity other than 4 and 8, an
 * unknown `of` or mode, SPLIT of zeros, run_offsets that decrease, n_comps < 0 -> MRCNN_ERR_SHAPE; an RLE that does not sum to its h*w
 * -> MRCNN_ERR_SHAPE, the message starts "rle_components:" / "rle_components_host:" / "rle_components_select:" /
 * "rle_components_select_host:" and names the lowest such k, nothing is written.  Argument errors are answered before a device is
 * looked for; no gfx950 device -> MRCNN_ERR_HIP from the device entries (no CPU fallback).
 * Not here: uniting or splitting across images, cutting wrongly chained components inside mrcnn_unite_tiles, labelling instance-id
 * or panoptic maps, filtering by shape other than area, rank and border (the measures are there to build a keep mask from),
 * 6-connectivity, a workgroup-local path for small RLEs. */
#define MRCNN_COMPONENTS_OF_ZEROS 0
#define MRCNN_COMPONENTS_OF_ONES 1
#define MRCNN_COMPONENTS_MERGE 0
#define MRCNN_COMPONENTS_SPLIT 1
MRCNN_API int mrcnn_rle_components(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                   int connectivity, int of, int memspace, int64_t* comp_offsets, uint32_t* comp_areas,
                                   int32_t* comp_bboxes_xywh, uint8_t* comp_flags, int64_t comp_capacity);
MRCNN_API int mrcnn_rle_components_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                        const int32_t* widths, int connectivity, int of, int64_t* comp_offsets, uint32_t* comp_areas,
                                        int32_t* comp_bboxes_xywh, uint8_t* comp_flags, int64_t comp_capacity);
MRCNN_API int mrcnn_rle_components_select(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                          const int32_t* widths, int connectivity, int of, const uint8_t* keep, int64_t n_comps, int mode,
                                          int memspace, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas,
                                          int32_t* bboxes_xywh, int64_t* out_parent, int64_t* out_n);
MRCNN_API int mrcnn_rle_components_select_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                               const int32_t* widths, int connectivity, int of, const uint8_t* keep, int64_t n_comps, int mode,
                                               uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas,
                                               int32_t* bboxes_xywh, int64_t* out_parent, int64_t* out_n);

/* ---- combining run-length masks: union, intersection, difference (csrc/api_rle_combine.hip, kernels_rle_combine.hip) ------------------
 * The set algebra of RLEs, the counterpart of pycocotools' mask.merge: RLE in, RLE out, no dense plane.  The set is flat as
 * mrcnn_rle_morph takes it: RLE k is counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane (sides
 * 1..32767); heights and widths are HOST arrays of n.  Zero-length runs are allowed anywhere.
 * The groups are HOST arrays in both memory spaces, like heights: group g combines the RLEs members[group_offsets[g] ..
 * group_offsets[g+1]) of the set, in that order, over the plane of its first member; every member must have that plane's height and
 * width.  group_offsets holds n_groups + 1 entries from 0 and does not decrease; no group is empty.  An RLE may be a member of any
 * number of groups, and of one group more than once.
 * The rule (csrc/combine_rule.h), pixel by pixel:
 *   MRCNN_RLE_OR    set in at least one member
 *   MRCNN_RLE_AND   set in every member
 *   MRCNN_RLE_XOR   set in an odd number of members (a member listed twice counts twice)
 *   MRCNN_RLE_DIFF  set in the first member and in none of the others (the first member listed again empties the result)
 * Outputs: one canonical RLE per group, exactly as mrcnn_rle_morph writes them (counts[0] may be 0, no other run is, runs continue
 * across column ends, an empty plane is the single run [h*w]).  out_run_offsets has n_groups + 1 entries and is always written;
 * areas (n_groups) and bboxes_xywh (n_groups, 4) are optional (NULL); the out_counts / capacity protocol with its size query is
 * mrcnn_rle_morph's: out_counts is written only when all runs fit, a smaller capacity -> MRCNN_ERR_SHAPE, the message names the
 * capacity needed (= out_run_offsets[n_groups]); capacity = 0 with out_counts = NULL is the size query.  memspace holds for counts,
 * run_offsets and the four outputs; the outputs must not overlap the inputs.  n_groups = 0 and n = 0 are legal: out_run_offsets[0] = 0.
 * mrcnn_rle_combine_host is the definition: sequential plain C++, no GPU, host pointers; one group at a time it decodes the first
 * member into a plane, folds every further member into it pixel by pixel, and encodes.  mrcnn_rle_combine equals it bit for bit in
 * every output array and never builds a plane: the prefix table of the runs and mrcnn_rle_morph's tight boxes (with the one flag that
 * refuses a wrong total) are read back once; the host sizes a packed bit box per group — the first member's tight box for AND and
 * DIFF, the hull of the members' boxes for OR and XOR; scratch that follows the masks, not the images — and uploads the member table;
 * one thread per column of a group's box folds the runs of that column of every member (one binary search per member, then a walk)
 * into its own column of words, kept in LDS, 1024 rows per pass: OR sets the intervals of ones, XOR toggles them, DIFF clears them, AND
 * clears the gaps between them; the encoder of mrcnn_masks_rle_source runs on the bits.  A thread owns its column: nothing is atomic
 * and the result does not depend on the order of execution.  The number of launches depends on neither n, n_groups nor the group sizes.
 * Errors, answered before a device is looked for, nothing written: null pointer, unknown memspace -> MRCNN_ERR_INVALID; an unknown
 * op, n or n_groups < 0, a side outside 1..32767, run_offsets that decrease, group_offsets[0] != 0 or decreasing group_offsets, an
 * empty group, a member outside 0..n-1, a member whose height or width differs from its group's first member (the message names the
 * group and the member) -> MRCNN_ERR_SHAPE.  An RLE of the set, referenced or not, that does not sum to its h*w -> MRCNN_ERR_SHAPE,
 * the message starts "rle_combine:" / "rle_combine_host:" and names the lowest such k, nothing is written.  No gfx950 device ->
 * MRCNN_ERR_HIP from the device entry (no CPU fallback).
 * Not here: a vote (set in at least m of K members), combining across planes of different sizes (mrcnn_rle_transform brings them
 * into one frame first: a = 1, d = 1, b = (-x0, -y0); rle_place in Python), group tables that live on the device, the complement (it
 * is XOR with a full mask, and a host can write the full mask [0, h*w]). */
#define MRCNN_RLE_OR 0
#define MRCNN_RLE_AND 1
#define MRCNN_RLE_XOR 2
#define MRCNN_RLE_DIFF 3
MRCNN_API int mrcnn_rle_combine(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                const int64_t* group_offsets, const int64_t* members, int64_t n_groups, int op, int memspace,
                                uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_rle_combine_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                     const int32_t* widths, const int64_t* group_offsets, const int64_t* members, int64_t n_groups, int op,
                                     uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh);

/* ---- moving run-length masks: crop, place, flip, rotate, resize (csrc/api_rle_transform.hip, kernels_rle_transform.hip) ---------------
 * A mask brought to another pixel grid: RLE in, RLE out, no dense plane.  The set is flat as mrcnn_rle_morph takes it: RLE k is
 * counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane P (sides 1..32767); heights and widths are
 * HOST arrays of n.  Zero-length runs are allowed anywhere.
 * Per RLE the caller gives an output plane and one record, all three HOST arrays in both memory spaces, like heights:
 *   out_heights[k], out_widths[k]     sides 1..32767
 *   xf[k] = [flags, ax, bx, dx, ay, by, dy, 0]     eight int64
 * The rule (csrc/transform_rule.h), for the output pixel (X, Y), column X and row Y:
 *   u = floor((ax*X + bx) / dx)        v = floor((ay*Y + by) / dy)        (floor towards -infinity, also for negatives)
 *   (sx, sy) = (u, v)                  or (v, u) when flags has MRCNN_XF_TRANSPOSE
 *   Out[Y, X] = P[sy, sx] if 0 <= sx < w and 0 <= sy < h, else 0
 * Limits: 1 <= dx, dy <= 2^31-1, 1 <= |ax|, |ay| <= 2^31-1, |bx|, |by| <= 2^46 — every product then stays inside int64.  Bits of
 * flags other than bit 0 must be 0; word 7 must be 0.  What the one rule covers:
 *   crop / window at (x0, y0)            a = 1, d = 1, b = (x0, y0); the window may reach outside the plane, and that part is 0
 *   place / pad / translate              a = 1, d = 1, b = (-x0, -y0) into a larger frame
 *   horizontal or vertical flip          a = -1, b = w-1 or h-1
 *   transpose, the four rotations        MRCNN_XF_TRANSPOSE with flips: the eight symmetries of the rectangle
 *   nearest resize, pixel-centre rule    src = floor((2X+1)*w / (2W')):  a = 2w, b = w, d = 2W'
 *   nearest resize, floor rule           src = floor(X*w / W'):  a = w, b = 0, d = W'
 *   any of these combined                one record: "crop this window and deliver it at half size, mirrored"
 * Outputs: one canonical RLE per input over its output plane, exactly as mrcnn_rle_morph writes them (counts[0] may be 0, no other
 * run is, runs continue across column ends, an empty plane is the single run [H'*W']).  out_run_offsets has n + 1 entries and is
 * always written; areas (n) and bboxes_xywh (n, 4) are optional (NULL); the out_counts / capacity protocol with its size query is
 * mrcnn_rle_morph's: out_counts is written only when all runs fit, a smaller capacity -> MRCNN_ERR_SHAPE, the message names the
 * capacity needed (= out_run_offsets[n]); capacity = 0 with out_counts = NULL is the size query.  memspace holds for counts,
 * run_offsets and the four outputs; the outputs must not overlap the inputs.  n = 0 is legal: out_run_offsets[0] = 0.
 * mrcnn_rle_transform_host is the definition: sequential plain C++, no GPU, host pointers; one RLE at a time it decodes the plane,
 * evaluates the forward rule above for every pixel of the output plane, and encodes.  mrcnn_rle_transform equals it bit for bit in
 * every output array and never builds a plane: the prefix table of the runs and mrcnn_rle_morph's tight boxes (with the one flag that
 * refuses a wrong total) are read back once; the host takes the preimage of every tight box under its record, clipped to the output
 * plane — the range of X with u(X) in [a, b) is [ceil((a*dx - bx)/ax), ceil((b*dx - bx)/ax)) for ax > 0 and
 * [floor((bx - b*dx)/(-ax)) + 1, floor((bx - a*dx)/(-ax)) + 1) for ax < 0 — and sizes a packed bit box per RLE from it: scratch that
 * follows the masks, not the images.  One thread per column of a box fills its own column of words, kept in LDS, 1024 rows per pass:
 * for a plain record it walks the runs of source column u(X) and sets the Y range of every interval of ones by the same inverse, a
 * run costs O(1) whatever the scale; for a transposed record column X is a source ROW, and the thread asks the prefix table one point
 * query (a binary search) per distinct source column along Y.  The encoder of mrcnn_masks_rle_source runs on the bits.  A thread
 * owns its column: nothing is atomic and the result does not depend on the order of execution.  The number of launches depends on
 * neither n nor the records.  A call whose boxes together pass MRCNN_XF_MAX_BOX_WORDS words of bits -> MRCNN_ERR_SHAPE naming the
 * number (device entry only): split the set.
 * Errors, answered before a device is looked for, nothing written: null pointer, unknown memspace -> MRCNN_ERR_INVALID; n < 0, a
 * side of a source or an output plane outside 1..32767, run_offsets that decrease, a record with an unknown flag bit, a coefficient
 * outside its limits or a non-zero word 7 (the message names the RLE) -> MRCNN_ERR_SHAPE.  An RLE that does not sum to its h*w ->
 * MRCNN_ERR_SHAPE, the message starts "rle_transform:" / "rle_transform_host:" and names the lowest such k, nothing is written.  No
 * gfx950 device -> MRCNN_ERR_HIP from the device entry (no CPU fallback).
 * Not here: rotation by other angles and general affine or projective warps, anti-aliased or area-weighted resampling (nearest
 * only), mapping of detection boxes, composing two records into one. */
#define MRCNN_XF_TRANSPOSE 1
#define MRCNN_XF_MAX_BOX_WORDS (1LL << 30)
MRCNN_API int mrcnn_rle_transform(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                  const int32_t* out_heights, const int32_t* out_widths, const int64_t* xf, int memspace,
                                  uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh);
MRCNN_API int mrcnn_rle_transform_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                       const int32_t* widths, const int32_t* out_heights, const int32_t* out_widths, const int64_t* xf,
                                       uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh);

/* ---- measuring run-length masks: moments, perimeter, convex hull, oriented box (csrc/api_rle_shape.hip, kernels_rle_shape.hip) --------
 * The shape of every mask of a flat RLE set, from the runs, no dense plane.  The set is flat as mrcnn_rle_morph takes it: RLE k is
 * counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane (sides 1..32767); heights and widths are HOST
 * arrays of n.  Zero-length runs are allowed anywhere; n = 0 is legal.  memspace holds for counts, run_offsets and the output arrays;
 * n_vertices is a host word in both memory spaces.  Geometry is mrcnn_rle_to_polygons': pixel (x, y) is the square [x, x+1] x [y, y+1],
 * y points down, a vertex is a pixel corner.  Everything is integer arithmetic: no floating point in any of the four entries.
 * mrcnn_rle_measure writes measures, n x MRCNN_MEASURE_WORDS int64 per RLE, over the set pixels with pixel INDICES (x, y):
 *   [S1, Sx, Sy, Sxx, Sxy, Syy, perimeter]     S1 the area, Sx = sum x, Sy = sum y, Sxx = sum x^2, Sxy = sum x*y, Syy = sum y^2
 * perimeter is the number of unit edges between a set pixel and an unset pixel or the outside of the plane: exactly the total edge
 * length of the rings mrcnn_rle_to_polygons traces for that RLE.  An empty mask is seven zeros.  Ranges: S1 <= 32767^2 < 2^30; Sx,
 * Sy < 32767^3 / 2 < 2^44; Sxx, Sxy, Syy < 32767^4 / 3 < 2^59 < 2^60; perimeter <= 4 * S1: every word fits int64.  Central moments
 * (S1 * Sxx - Sx^2) do NOT fit 64 bits: a caller takes them in wider integers or in doubles from exactly reduced terms.
 * mrcnn_rle_convex_hull.  The hull of RLE k is the convex hull of its set pixels' SQUARES, a ring in the tracer's convention: integer
 * corner vertices, strictly convex (no vertex lies on a segment between two others), clockwise on screen with positive shoelace area,
 * starting at its smallest vertex by x then y: the top chain from (xmin, T) to (xmax+1, T') in rising x, then the bottom chain back in
 * falling x.  A non-empty mask has at least 4 hull vertices, an empty one none.  The hull is unique.
 *   hull_offsets (n + 1, int64)   always written: RLE k owns the vertices hull_offsets[k] .. hull_offsets[k+1]
 *   *n_vertices (host)            always written: hull_offsets[n]
 *   hull_areas2 (n int64, or NULL)  twice the hull's area; written whatever the capacity
 *   obb (n x 8 int64, or NULL)      the oriented box, below; written whatever the capacity
 *   xy (2 x vertex_capacity int32)  x, y per vertex, under mrcnn_polygons_simplify's capacity protocol: written only when all vertices
 *                                   fit, otherwise MRCNN_ERR_SHAPE and the message names the size needed; vertex_capacity = 0 with
 *                                   xy = NULL is the size query.
 * The oriented box is the minimum-area rectangle around the hull, one side on a hull edge, exact in integers.  For hull edge e from
 * v_e to v_{e+1} (cyclic) with (dx, dy) its vector and L2 = dx^2 + dy^2, over all hull vertices (X, Y): d = dx*X + dy*Y and
 * c = dx*Y - dy*X, D = dmax - dmin, C = cmax - cmin; the rectangle's area is D*C / L2.  The chosen edge minimises it — two edges are
 * compared as D_i*C_i*L2_j < D_j*C_j*L2_i in 128 bits (94 are needed) — and a tie goes to the smallest e.  The row is
 * [e, dx, dy, dmin, dmax, cmin, cmax, 0] with e local to the RLE's hull, [-1, 0, ...] for an empty mask.  The point with coordinates
 * (d, c) is ((d*dx - c*dy) / L2, (d*dy + c*dx) / L2): a caller makes corners, centre, size and angle from that in doubles.
 * The _host entries are the definition: sequential plain C++, no GPU, host pointers; one RLE at a time the runs are cut into column
 * pieces (touching pieces joined), the moments are summed pixel by pixel, the perimeter is counted from the pieces of neighbouring
 * columns, the hull is Andrew's monotone chain over the columns' first and last set rows and the box the loop over edges x vertices.
 * The device entries equal them bit for bit in every output array and never build a plane.  Moments: one block per RLE strides over
 * the runs of ones of rle_prefix_forward's table; a run is a head piece, a block of full columns and a tail piece, each a closed form
 * in its ends, so a full plane costs what one pixel costs.  Perimeter: one thread per vertex column X = 0 .. w, one binary search
 * per pixel column and the merge of columns X - 1 and X: the rows where they differ (outside the plane is empty) plus 2 per piece of
 * column X, added to the RLE's word by 64-bit integer atomics.  Hull: one thread per pixel column finds the first and last set row;
 * vertex column X takes the smaller first and the larger last row of its non-empty neighbours (empty columns inside a mask are
 * skipped); one workgroup per RLE runs QuickHull level by level on both chains at once — a 64-bit maximum per chain segment of
 * c(p) = (by-ay)(px-ax) - (bx-ax)(py-ay) picks a candidate, a tie goes to the smallest position in walking order, it is kept only if
 * c > 0, the loop ends when no segment is left — in LDS up to MRCNN_HULL_LDS_COLUMNS vertex columns (32 bytes per column: 128 KiB),
 * in global scratch above; the counts are scanned, the rings written with their areas, and one workgroup per RLE with one thread per
 * hull edge finds the box by a block-wide 128-bit minimum.  The host reads back one flag before anything is written (an RLE that does
 * not sum to its plane) and *n_vertices after the count; the number of launches depends on neither n nor the hulls' sizes.
 * Errors, answered before a device is looked for, nothing written: null pointer, unknown memspace, negative vertex_capacity, null xy
 * with a capacity -> MRCNN_ERR_INVALID; n < 0, a side outside 1..32767, run_offsets that decrease -> MRCNN_ERR_SHAPE.  An RLE that does
 * not sum to its h*w -> MRCNN_ERR_SHAPE, the message starts "rle_measure:" / "rle_measure_host:" / "rle_convex_hull:" /
 * "rle_convex_hull_host:" and names the lowest such k, nothing is written.  No gfx950 device -> MRCNN_ERR_HIP from the device entries
 * (no CPU fallback).
 * Not here: Feret diameters, Hu moments, hulls of rings, boxes under other criteria (smallest perimeter, axis of inertia), measures
 * per connected component in one call (mrcnn_rle_components_select's SPLIT output feeds these entries as it is). */
#define MRCNN_MEASURE_WORDS 7
#define MRCNN_HULL_LDS_COLUMNS 4096
MRCNN_API int mrcnn_rle_measure(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                int memspace, int64_t* measures);
MRCNN_API int mrcnn_rle_measure_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                     const int32_t* widths, int64_t* measures);
MRCNN_API int mrcnn_rle_convex_hull(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                    int memspace, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy, int64_t* n_vertices,
                                    int64_t vertex_capacity);
MRCNN_API int mrcnn_rle_convex_hull_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                         const int32_t* widths, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy,
                                         int64_t* n_vertices, int64_t vertex_capacity);

#ifdef __cplusplus
}
#endif
#endif /* MASKRCNN_HIP_H */
