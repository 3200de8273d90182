// engine.hip — the run-time side of the three models that replace the Core ML graph executors of MaskRCNN.mlmodel, Classifier.mlmodel
// and Mask.mlmodel (reference: Sources/maskrcnn/Python/Conversion/task.py:69-116 emits the specs; the layer list itself is the Matterport
// layout of the un-vendored `maskrcnn` package): errors, the roctx binding, the stage timer, the four predict
// entries, the two-slot pipeline and read_tensor.  The rest of the engine: engine_weights.hip (artefacts → packed weights),
// engine_heads.hip (the box and mask heads), engine_plan.hip (Model::load and the trunk's plan), engine_split.hip (split exponents).
//
// HBM layout: activations NHWC in the compute mode's element type (fp16 in MRCNN_F16; fp32 in MRCNN_F32 and in the split modes, whose
// tensors are stored as 2^e * value, engine.h: SplitGroup) in one arena, one dense tensor per layer output except where a stage reuses
// its branch tensors and writes its block outputs in place (engine_plan.hip); a batch of 8 × 1024² images needs a few GB of the 288 GB.
// Filters are packed once at load as [Npad][tap][cin] in the mode's filter type (fp32, or fp16 in MRCNN_F16 and the split modes), some
// layers also in the re-tiled orders of the halo, 3x3-fp16 and fused-bottleneck kernels (engine.h: PackedConv), with BatchNorm folded
// into a per-channel fp32 scale / shift.  The pyramid P2..P5 stays resident for both ROIAlign passes (the reference re-uploads 89 MB of
// textures per call, PyramidROIAlignLayer.swift:110-118).
#include <dlfcn.h>

#include "engine_internal.h"
#include "knobs.h"

#include <math.h>
#include <stdarg.h>
#include <string.h>

namespace mrcnn {

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

void set_error(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}
const char* last_error() { return g_last_error.c_str(); }

// ---- roctx (run-time bound) ----------------------------------------------------------------------------------------
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char* e = getenv("MRCNN_ROCTX");
        if (e && atoi(e) == 0) return;
        for (const char* n : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void* h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            auto pu = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            auto po = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (pu && po) { push = pu; pop = po; return; }
        }
    }
};
Roctx& roctx() { static Roctx r; return r; }
}  // namespace
void trace_push(const char* name) { if (roctx().push) (void)roctx().push(name); }
void trace_pop() { if (roctx().pop) (void)roctx().pop(); }

void fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, buf};
}

void require_gpu()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        fail(MRCNN_ERR_HIP, "no HIP device visible (%s): libmaskrcnn_hip has no CPU fallback",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIP_CHECK(hipGetDeviceProperties(&p, dev));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        fail(MRCNN_ERR_HIP, "device %d is %s; this library is built for gfx950 (MI355X) only", dev, p.gcnArchName);
}

// ------------------------------------------------------------------------------------------------
// timers
// ------------------------------------------------------------------------------------------------
void StageTimer::begin(hipStream_t s)
{
    if (!enabled) return;
    names.clear();
    if (ev.empty()) {
        ev.resize(16);
        for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    }
    HIP_CHECK(hipEventRecord(ev[0], s));
}
void StageTimer::mark(hipStream_t s, const char* name)
{
    if (!enabled) return;
    names.push_back(name);
    HIP_CHECK(hipEventRecord(ev[names.size()], s));
}
void StageTimer::finish()
{
    if (!enabled || names.empty()) return;
    HIP_CHECK(hipEventSynchronize(ev[names.size()]));
    ms.clear();
    for (size_t i = 0; i < names.size(); ++i) {
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
        ms[names[i]] = t;
    }
}
StageTimer::~StageTimer()
{
    for (auto& e : ev) (void)hipEventDestroy(e);
}

// ------------------------------------------------------------------------------------------------
// Model
// ------------------------------------------------------------------------------------------------
void Model::drop_graphs()
{
    for (auto& kv : graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    graphs.clear();
}

Model::~Model()
{
    drop_graphs();
    for (auto& sl : pipe) {
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (pipe_in) (void)hipStreamDestroy(pipe_in);
    if (pipe_out) (void)hipStreamDestroy(pipe_out);
    if (ev_p0) (void)hipEventDestroy(ev_p0);
    if (ev_p1) (void)hipEventDestroy(ev_p1);
    if (fit_pack) (void)hipHostFree(fit_pack);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

// bit 1 of the range flag: the verdict of the whole-stage bottleneck launch's own watchdog (predict and collect word it alike)
static const char kStageStalled[] =
    "a whole-stage bottleneck launch made no progress for ~0.1 s (its grid was not resident as a whole: are compute units masked off or "
    "held by another process?): the results of this call are not valid; mrcnn_debug_set(\"conv_bneck_stage\", 0) runs one launch per block";

void Model::predict(const uint8_t* rgb, int batch, int h, int w, int memspace, float* det_out, float* masks_out, bool sync, bool fit, bool resident)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "predict called on a non-MaskRCNN model");
    MRCNN_REQUIRE((rgb || resident) && ((det_out && masks_out) || calib_phase), MRCNN_ERR_INVALID, "null buffer");
    MRCNN_REQUIRE(fit ? (h > 0 && w > 0 && h < 32768 && w < 32768) : (h == H && w == W), MRCNN_ERR_SHAPE,
                  "image is %dx%d, the model expects %dx%d (mrcnn_maskrcnn_predict_scalefit letterboxes any size)", h, w, H, W);
    MRCNN_REQUIRE(batch >= 1 && batch <= max_batch, MRCNN_ERR_SHAPE, "batch %d outside 1..%d", batch, max_batch);
    hipStream_t s = stream;
    int fitgeo[6] = {h, w, 0, 0, 0, 0};
    if (fit && !fit_mixed) {      // (predict_images has staged its images and their geometry table already)
        MRCNN_REQUIRE(mrcnn_letterbox_geometry(h, w, H, W, &fitgeo[2], &fitgeo[3], &fitgeo[4], &fitgeo[5]) == MRCNN_OK, MRCNN_ERR_INVALID, "bad letterbox geometry");
        const size_t need = (size_t)batch * h * w * 3;
        if (fit_src.bytes < need) { HIP_CHECK(hipStreamSynchronize(s)); fit_src.alloc(need); drop_graphs(); }
    }
    const size_t img_bytes = (size_t)batch * h * w * 3;
    uint8_t* const img_dst = fit ? fit_src.as<uint8_t>() : d_rgb;
    if (!ev_p0) { HIP_CHECK(hipEventCreate(&ev_p0)); HIP_CHECK(hipEventCreate(&ev_p1)); }
    hipStreamCaptureStatus outer_capture = hipStreamCaptureStatusNone;
    HIP_CHECK(hipStreamIsCapturing(s, &outer_capture));
    const bool timed_call = sync && outer_capture == hipStreamCaptureStatusNone;
    if (timed_call) HIP_CHECK(hipEventRecord(ev_p0, s));
    if (!resident) HIP_CHECK(hipMemcpyAsync(img_dst, rgb, img_bytes, memspace == MRCNN_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));

    hipStreamCaptureStatus caller_capture = hipStreamCaptureStatusNone;
    if (use_graph) HIP_CHECK(hipStreamIsCapturing(s, &caller_capture));
    // (the scale-fit geometry is a launch argument of the first kernel: such calls are not replayed from a captured graph)
    const bool plain = !use_graph || fit || timer.enabled || conv_profile.active || calib_phase || caller_capture != hipStreamCaptureStatusNone;
    if (plain) {
        enqueue_pipeline(s, batch, fit ? fitgeo : nullptr);
    } else {
        GraphSlot& g = graphs[batch];
        if (!g.exec && g.eager_runs++ == 0) {
            enqueue_pipeline(s, batch);              // first call at this batch size: also runs the one-time host set-up
        } else {
            if (!g.exec) {
                HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                try {
                    enqueue_pipeline(s, batch);
                } catch (...) {
                    hipGraph_t dead = nullptr;
                    (void)hipStreamEndCapture(s, &dead);
                    if (dead) (void)hipGraphDestroy(dead);
                    throw;
                }
                HIP_CHECK(hipStreamEndCapture(s, &g.graph));
                HIP_CHECK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
            }
            HIP_CHECK(hipGraphLaunch(g.exec, s));
            ++graph_launches;
        }
    }

    const int HW = 4 * mask_pool * mask_pool;
    // (the recovery path of collect() reads device images and writes host records: the direction of the record copies follows the pointers)
    auto copy_records = [&] {
        if (det_out) HIP_CHECK(hipMemcpyAsync(det_out, detections, (size_t)batch * max_det * 6 * 4, hipMemcpyDefault, s));
        if (masks_out) HIP_CHECK(hipMemcpyAsync(masks_out, mask_out, (size_t)batch * max_det * HW * 4, hipMemcpyDefault, s));
    };
    copy_records();
    if (timed_call) HIP_CHECK(hipEventRecord(ev_p1, s));
    if (sync) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (timed_call && !calib_phase) {              // (calibration / recovery passes are not the host's predicts)
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ev_p0, ev_p1));
            gpu_busy_ms += ms;
            ++predict_calls;
        }
        timer.finish();
        if (conv_profile.active) conv_profile.collect();
        if (mode != MRCNN_F32) {
            int tripped = 0;
            HIP_CHECK(hipMemcpy(&tripped, range_flag.p, sizeof(int), hipMemcpyDeviceToHost));
            if (tripped & 2) fail(MRCNN_ERR_HIP, "%s", kStageStalled);
            if (tripped && calib_phase)
                fail(MRCNN_ERR_UNSUPPORTED, "an activation left the fp16 range during a calibration pass");       // (the caller steps the exponents down)
            if (tripped) {
                ++range_overflows;
                // split modes: this batch needs smaller exponents than the calibration images did — measure it where it sits, lower them,
                // compute it again.  The reference's fp32 path handles any such input (Conversion/task.py:90).
                if (outer_capture == hipStreamCaptureStatusNone && recover_range(batch, h, w, fit)) {
                    ++range_recoveries;
                    enqueue_pipeline(s, batch, fit ? fitgeo : nullptr);
                    copy_records();
                    HIP_CHECK(hipStreamSynchronize(s));
                    timer.finish();
                    if (conv_profile.active) conv_profile.collect();
                    HIP_CHECK(hipMemcpy(&tripped, range_flag.p, sizeof(int), hipMemcpyDeviceToHost));
                    if (!tripped) return;
                }
                fail(MRCNN_ERR_UNSUPPORTED, "an activation left the fp16 range (|v| >= 65504) in compute mode %s: the results of this call are "
                     "not valid; load the model with MRCNN_F32", mode == MRCNN_F16 ? "MRCNN_F16" : (mode == MRCNN_F32S ? "MRCNN_F32S" : "MRCNN_F32X3"));
            }
        }
    }
}

void Model::predict_images(const mrcnn_image* images, int batch, int memspace, float* det_out, float* masks_out)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "predict_images called on a non-MaskRCNN model");
    MRCNN_REQUIRE(images && det_out && masks_out, MRCNN_ERR_INVALID, "null buffer");
    MRCNN_REQUIRE(batch >= 1 && batch <= max_batch, MRCNN_ERR_SHAPE, "batch %d outside 1..%d", batch, max_batch);
    std::vector<ImageGeom> geom((size_t)batch);
    size_t need = 0;
    for (int b = 0; b < batch; ++b) {
        const mrcnn_image& im = images[b];
        MRCNN_REQUIRE(im.rgb, MRCNN_ERR_INVALID, "image %d of the batch: null rgb pointer", b);
        MRCNN_REQUIRE(im.height >= 1 && im.height <= 32767 && im.width >= 1 && im.width <= 32767, MRCNN_ERR_SHAPE,
                      "image %d of the batch is %dx%d: height and width must lie in 1..32767", b, im.height, im.width);
        ImageGeom& g = geom[(size_t)b];
        g.offset = (long long)need; g.h = im.height; g.w = im.width; g.pitch = g.w;
        MRCNN_REQUIRE(mrcnn_letterbox_geometry(g.h, g.w, H, W, &g.nh, &g.nw, &g.py, &g.px) == MRCNN_OK, MRCNN_ERR_INVALID,
                      "image %d of the batch: bad letterbox geometry", b);
        need += (size_t)g.h * g.w * 3;
    }
    hipStream_t s = stream;
    const size_t table_off = (need + 15) & ~(size_t)15, table_bytes = (size_t)batch * sizeof(ImageGeom), total = table_off + table_bytes;
    if (fit_src.bytes < total) { HIP_CHECK(hipStreamSynchronize(s)); fit_src.alloc(total); drop_graphs(); }
    if (fit_pack_bytes < table_bytes) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (fit_pack) { (void)hipHostFree(fit_pack); fit_pack = nullptr; fit_pack_bytes = 0; }
        const size_t cap = (size_t)max_batch * sizeof(ImageGeom);
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&fit_pack), cap, hipHostMallocDefault));
        fit_pack_bytes = cap;
    }
    // whatever way the call is left, the stream has drained before it returns (the copies below read fit_pack and the caller's
    // images) and the handle is back in its plain state
    struct Leave {
        Model* m;
        ~Leave() { (void)hipStreamSynchronize(m->stream); m->fit_mixed = false; }
    } leave{this};
    fit_table_off = table_off;
    fit_mixed = true;
    uint8_t* const dst = fit_src.as<uint8_t>();
    memcpy(fit_pack, geom.data(), table_bytes);
    HIP_CHECK(hipMemcpyAsync(dst + table_off, fit_pack, table_bytes, hipMemcpyHostToDevice, s));
    // (the images go straight from the caller's memory, one copy each: packing 10 MB of host images into a pinned buffer first was
    // measured SLOWER — 19.5 against 18.8 ms per batch-8 step — than letting the runtime pin and copy each)
    const hipMemcpyKind in = memspace == MRCNN_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int b = 0; b < batch; ++b)
        HIP_CHECK(hipMemcpyAsync(dst + geom[(size_t)b].offset, images[b].rgb, (size_t)geom[(size_t)b].h * geom[(size_t)b].w * 3, in, s));
    predict(nullptr, batch, H, W, MRCNN_DEVICE, det_out, masks_out, true, true, true);
}

void Model::predict_tiles(const mrcnn_image* images, int n_images, const mrcnn_tile* tiles, int n_tiles, int memspace, float* det_out, float* masks_out)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "predict_tiles called on a non-MaskRCNN model");
    MRCNN_REQUIRE(images && tiles && det_out && masks_out, MRCNN_ERR_INVALID, "null buffer");
    const bool dev = memspace == MRCNN_DEVICE;
    // host images: back to back in fit_src, each from a 16-byte boundary; device images are read where they lie — an entry's offset
    // is then the distance of its first byte from fit_src (one flat address space: k_preprocess_images only adds it to that base)
    std::vector<size_t> at((size_t)n_images, 0);
    size_t need = 0;
    if (!dev)
        for (int b = 0; b < n_images; ++b) { at[(size_t)b] = need; need += ((size_t)images[b].height * images[b].width * 3 + 15) & ~(size_t)15; }
    hipStream_t s = stream;
    const size_t table_off = (need + 15) & ~(size_t)15, cap = (size_t)max_batch * sizeof(ImageGeom), total = table_off + cap;
    if (fit_src.bytes < total) { HIP_CHECK(hipStreamSynchronize(s)); fit_src.alloc(total); drop_graphs(); }
    if (fit_pack_bytes < cap) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (fit_pack) { (void)hipHostFree(fit_pack); fit_pack = nullptr; fit_pack_bytes = 0; }
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&fit_pack), cap, hipHostMallocDefault));
        fit_pack_bytes = cap;
    }
    struct Leave {
        Model* m;
        ~Leave() { (void)hipStreamSynchronize(m->stream); m->fit_mixed = false; }
    } leave{this};
    fit_table_off = table_off;
    fit_mixed = true;
    uint8_t* const dst = fit_src.as<uint8_t>();
    if (!dev)
        for (int b = 0; b < n_images; ++b)
            HIP_CHECK(hipMemcpyAsync(dst + at[(size_t)b], images[b].rgb, (size_t)images[b].height * images[b].width * 3, hipMemcpyHostToDevice, s));
    const int HW = 4 * mask_pool * mask_pool;
    for (int t0 = 0; t0 < n_tiles; t0 += max_batch) {
        const int n = n_tiles - t0 < max_batch ? n_tiles - t0 : max_batch;
        ImageGeom* const geom = reinterpret_cast<ImageGeom*>(fit_pack);       // (the predict before this one has drained the stream)
        for (int i = 0; i < n; ++i) {
            const mrcnn_tile& w = tiles[t0 + i];
            const mrcnn_image& im = images[w.image];
            ImageGeom& g = geom[i];
            const long long first = ((long long)w.y0 * im.width + w.x0) * 3;
            g.offset = dev ? (long long)(reinterpret_cast<intptr_t>(im.rgb) - reinterpret_cast<intptr_t>(dst)) + first : (long long)at[(size_t)w.image] + first;
            g.h = w.height; g.w = w.width; g.pitch = im.width;
            MRCNN_REQUIRE(mrcnn_letterbox_geometry(g.h, g.w, H, W, &g.nh, &g.nw, &g.py, &g.px) == MRCNN_OK, MRCNN_ERR_INVALID,
                          "tile %d: bad letterbox geometry", t0 + i);
        }
        HIP_CHECK(hipMemcpyAsync(dst + table_off, fit_pack, (size_t)n * sizeof(ImageGeom), hipMemcpyHostToDevice, s));
        predict(nullptr, n, H, W, MRCNN_DEVICE, det_out + (size_t)t0 * max_det * 6, masks_out + (size_t)t0 * max_det * HW, true, true, true);
    }
}

// ---- pipelined host entry ------------------------------------------------------------------------------------------------
void Model::submit(const uint8_t* rgb_host, int batch, int h, int w)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "submit called on a non-MaskRCNN model");
    MRCNN_REQUIRE(rgb_host, MRCNN_ERR_INVALID, "null buffer");
    MRCNN_REQUIRE(h == H && w == W, MRCNN_ERR_SHAPE, "image is %dx%d, the model expects %dx%d", h, w, H, W);
    MRCNN_REQUIRE(batch >= 1 && batch <= max_batch, MRCNN_ERR_SHAPE, "batch %d outside 1..%d", batch, max_batch);
    MRCNN_REQUIRE(pipe_submitted - pipe_collected < 2, MRCNN_ERR_INVALID, "two batches are in flight already: call mrcnn_maskrcnn_collect first");
    // the stage timer and the conv profile hold ONE batch's events: a second submission would re-record what the first one's collect reads
    MRCNN_REQUIRE(pipe_submitted == pipe_collected || !(timer.enabled || conv_profile.active), MRCNN_ERR_INVALID,
                  "stage timing / the conv profile are on: collect the batch in flight before submitting the next");
    PipeSlot& sl = pipe[pipe_submitted & 1];
    const int HW = 4 * mask_pool * mask_pool;
    if (!pipe_in) {
        HIP_CHECK(hipStreamCreateWithFlags(&pipe_in, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&pipe_out, hipStreamNonBlocking));
    }
    if (!sl.ev_in) {
        HIP_CHECK(hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
        sl.rgb.alloc((size_t)max_batch * H * W * 3);
        sl.det.alloc((size_t)max_batch * max_det * 6 * 4);
        sl.mask.alloc((size_t)max_batch * max_det * HW * 4);
        sl.flag.alloc(sizeof(int));
    }
    hipStream_t s = stream;
    // the images cross PCIe on the copy stream (under whatever the compute stream is doing: the previous batch's predict) ...
    HIP_CHECK(hipMemcpyAsync(sl.rgb.p, rgb_host, (size_t)batch * H * W * 3, hipMemcpyHostToDevice, pipe_in));
    HIP_CHECK(hipEventRecord(sl.ev_in, pipe_in));
    // ... and the compute stream picks them up when they have arrived
    HIP_CHECK(hipStreamWaitEvent(s, sl.ev_in, 0));
    HIP_CHECK(hipMemcpyAsync(d_rgb, sl.rgb.p, (size_t)batch * H * W * 3, hipMemcpyDeviceToDevice, s));
    enqueue_pipeline(s, batch);
    HIP_CHECK(hipMemcpyAsync(sl.det.p, detections, (size_t)batch * max_det * 6 * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(sl.mask.p, mask_out, (size_t)batch * max_det * HW * 4, hipMemcpyDeviceToDevice, s));
    if (mode != MRCNN_F32) HIP_CHECK(hipMemcpyAsync(sl.flag.p, range_flag.p, sizeof(int), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipEventRecord(sl.ev_done, s));
    sl.batch = batch;
    sl.busy = true;
    ++pipe_submitted;
}

void Model::collect(float* det_host, float* masks_host, int* batch_out)
{
    MRCNN_REQUIRE(det_host && masks_host, MRCNN_ERR_INVALID, "null buffer");
    MRCNN_REQUIRE(pipe_submitted > pipe_collected, MRCNN_ERR_INVALID, "nothing was submitted");
    PipeSlot& sl = pipe[pipe_collected & 1];
    const int HW = 4 * mask_pool * mask_pool;
    int tripped = 0;
    // whatever happens below, the slot is handed back: a HIP error here must not leave it "in flight" for ever
    struct Release {
        Model* m; PipeSlot* sl;
        ~Release() { sl->busy = false; ++m->pipe_collected; }
    } release{this, &sl};
    HIP_CHECK(hipStreamWaitEvent(pipe_out, sl.ev_done, 0));
    HIP_CHECK(hipMemcpyAsync(det_host, sl.det.p, (size_t)sl.batch * max_det * 6 * 4, hipMemcpyDeviceToHost, pipe_out));
    HIP_CHECK(hipMemcpyAsync(masks_host, sl.mask.p, (size_t)sl.batch * max_det * HW * 4, hipMemcpyDeviceToHost, pipe_out));
    if (mode != MRCNN_F32) HIP_CHECK(hipMemcpyAsync(&tripped, sl.flag.p, sizeof(int), hipMemcpyDeviceToHost, pipe_out));
    HIP_CHECK(hipStreamSynchronize(pipe_out));
    if (pipe_submitted == pipe_collected + 1) {      // nothing newer has been enqueued: the stage timer / conv profile hold THIS batch's events
        timer.finish();
        if (conv_profile.active) conv_profile.collect();
    }
    if (batch_out) *batch_out = sl.batch;
    ++predict_calls;
    if (tripped & 2) fail(MRCNN_ERR_HIP, "%s", kStageStalled);
    if (tripped) {
        ++range_overflows;
        if (mode == MRCNN_F32S || mode == MRCNN_F32X3) {
            // this slot's images are still on the device: compute the batch again through the synchronous entry, which lowers the exponents
            // it needs (a newer batch already in flight was computed with the old ones and is checked at its own collect)
            --predict_calls;
            HIP_CHECK(hipStreamSynchronize(stream));                // (a newer batch in flight has finished: its records wait in its own slot)
            HIP_CHECK(hipMemcpyAsync(d_rgb, sl.rgb.p, (size_t)sl.batch * H * W * 3, hipMemcpyDeviceToDevice, stream));
            if (recover_range(sl.batch, H, W, false)) {
                ++range_recoveries;
                predict(nullptr, sl.batch, H, W, MRCNN_DEVICE, det_host, masks_host, true, false, true);
                return;
            }
        }
        fail(MRCNN_ERR_UNSUPPORTED, "an activation left the fp16 range (|v| >= 65504) in the fp16 compute mode: the results of this batch are "
             "not valid; load the model with MRCNN_F32X3 or MRCNN_F32");
    }
}

// process-wide A/B switch of the fused mask tail (tests, tools/e2e_ab.py): mrcnn_debug_set("mask_fused", 0 | 1)
static int& g_fuse_mask_tail = knob("mask_fused", nullptr, 1);

void Model::enqueue_pipeline(hipStream_t s, int batch, const int* fit)
{
    int* const rflag = mode != MRCNN_F32 ? range_flag.as<int>() : nullptr;
    if (rflag) HIP_CHECK(hipMemsetAsync(rflag, 0, sizeof(int), s));
    // the thread-local hand-overs of the convolution family (range flag, scratch, profiler) point into THIS model: whatever way the
    // function is left — a launch may throw — they are cleared, so that nothing dangles once the handle is destroyed
    struct LaunchContext {
        ~LaunchContext() { conv_set_profiler(nullptr); conv_set_range_flag(nullptr); conv_set_scratch(nullptr); }
    } launch_context;
    conv_set_range_flag(rflag);
    conv_set_scratch(conv_scratch.ks_buf.p ? &conv_scratch : nullptr);
    timer.begin(s);
    conv_set_profiler(conv_profile.active ? &conv_profile : nullptr);
    {
        TraceRange tr("MaskRCNN-Trunk");          // the Core ML graph itself: no signpost in the reference
        size_t first = 0;
        if (fit) {      // .scaleFit: letterbox + mean subtraction in one kernel, instead of trunk_ops[0] (d_rgb → stem_in)
            if (fit_mixed) preprocess_images_forward(s, fit_src.as<uint8_t>(), reinterpret_cast<const ImageGeom*>(fit_src.as<uint8_t>() + fit_table_off), batch, H, W, 3, mean, stem_in, dtype);
            else preprocess_scalefit_forward(s, fit_src.as<uint8_t>(), batch, fit[0], fit[1], H, W, fit[2], fit[3], fit[4], fit[5], 3, mean, stem_in, dtype);
            first = 1;
        }
        for (size_t i = first; i < trunk_ops.size(); ++i) trunk_ops[i](s, batch);
    }
    timer.mark(s, "Trunk");
    // ProposalLayer
    ProposalWorkspace pw = prop_ws; pw.B = batch;
    {
        TraceRange tr("Proposal-Eval");
        proposal_forward(s, pw, rpn_probs, (long)A * 2, rpn_deltas, (long)A * 4, anchors.as<float>(), prop_std, prop_nms_thr, rois,
                         (long)max_prop * 4, 4);
    }
    timer.mark(s, "Proposal-Eval");
    // PyramidROIAlign (classifier)
    PyramidMaps maps;
    for (int l = 0; l < 4; ++l) { maps.data[l] = P[l].p; maps.H[l] = P[l].H; maps.W[l] = P[l].W; maps.sB[l] = P[l].sB(); }
    // the pyramid levels may sit at different split exponents: the sampler brings each to the exponent of its output (exact)
    auto level_muls = [&](int g_out) { for (int l = 0; l < 4; ++l) maps.mul[l] = ldexpf(1.0f, sgroups[(size_t)g_out].exp - sgroups[(size_t)g_P[l]].exp); };
    const long prow = (long)cls_pool * cls_pool * 256;
    {
        TraceRange tr("PyramidROIAlign-Eval");
        level_muls(g_pooled);
        roi_align_forward(s, maps, 256, 1, rois, (long)max_prop * 4, 4, max_prop, batch, cls_pool, roi_img_w, roi_img_h, pooled,
                          (long)max_prop * prow, prow, dtype);
        if (calib_phase) observe_split(s, g_pooled, pooled, (size_t)batch * max_prop * prow);
    }
    timer.mark(s, "PyramidROIAlign-Eval");
    // TimeDistributedClassifier
    {
        TraceRange tr("TimeDistributedClassifierLayer-Eval");
        cls_head.forward(s, pooled, batch * max_prop, cls6, 6);
    }
    timer.mark(s, "TimeDistributedClassifierLayer-Eval");
    // DetectionLayer
    DetectionWorkspace dw = det_ws; dw.B = batch;
    {
        TraceRange tr("Detection-Eval");
        detection_forward(s, dw, rois, (long)max_prop * 4, 4, cls6, (long)max_prop * 6, det_std, det_score_thr, det_nms_thr, nc,
                          detections, (long)max_det * 6, 6);
    }
    timer.mark(s, "Detection-Eval");
    // PyramidROIAlign (mask) on the detections' boxes
    const long mrow = (long)mask_pool * mask_pool * 256;
    // ... which also evaluates the mask layer's removeZeros predicate on the fp32 samples (before an fp16 store rounds them)
    {
        TraceRange tr("PyramidROIAlign-Eval");
        level_muls(g_pooled_mask);
        roi_align_forward(s, maps, 256, 1, detections, (long)max_det * 6, 6, max_det, batch, mask_pool, roi_img_w, roi_img_h, pooled_mask,
                          (long)max_det * mrow, mrow, dtype, msel_ws.flags);
        if (calib_phase) observe_split(s, g_pooled_mask, pooled_mask, (size_t)batch * max_det * mrow);
    }
    timer.mark(s, "PyramidROIAlign-Eval-Mask");
    // TimeDistributedMask
    TraceRange tr_mask("TimeDistributedMask-Eval");
    const int HW = 4 * mask_pool * mask_pool;
    mask_valid_rows_forward(s, nullptr, (long)max_det * mrow, mrow, mrow, max_det, batch, msel_ws, dtype);
    // Rows the reference's mask layer never writes (an invalid row below the kept count,
    // TimeDistributedMaskLayer.swift:58-89) hold whatever Core ML's buffer held; here they are defined: zero.
    HIP_CHECK(hipMemsetAsync(mask_out, 0, (size_t)batch * max_det * HW * sizeof(float), s));
    const bool fused_tail = fuse_mask_tail && g_fuse_mask_tail && mask_head.deconv.Cout % 128 == 0;
    if (fused_tail) {
        // the deconvolution's epilogue takes the dot with the selected class's 1x1 filter: its 256-channel output (642 MB of
        // fp32 per batch of 8) is never written nor read back
        mask_select_classes(s, detections, (long)max_det * 6, 6, max_det, batch, nc, msel_ws, msel_ws.sel_cid);
        mask_head.forward_features(s, pooled_mask, batch * max_det, msel_ws.sel_cid, mask_partial);
        mask_select_from_partials(s, mask_partial, mask_head.deconv.Cout / conv_sel_part_cols(), HW, mask_head.final_b.as<float>(), nc, detections,
                                  (long)max_det * 6, 6, max_det, batch, msel_ws, mask_out, (long)max_det * HW, HW);
    } else {
        mask_head.forward_features(s, pooled_mask, batch * max_det);
        mask_select_forward(s, mask_head.feat, (long)max_det * HW * mask_head.deconv.Cout, HW, mask_head.deconv.Cout,
                            mask_head.final_w.as<float>(), mask_head.final_b.as<float>(), nc, detections, (long)max_det * 6, 6, max_det,
                            batch, msel_ws, mask_out, (long)max_det * HW, HW, dtype);
    }
    timer.mark(s, "TimeDistributedMask-Eval");
}

void Model::read_tensor(const std::string& name, int image, float* dst, int64_t cap, int64_t* count)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "taps exist on the MaskRCNN model only");
    MRCNN_REQUIRE(image >= 0 && image < max_batch, MRCNN_ERR_INVALID, "image index %d out of range", image);
    HIP_CHECK(hipStreamSynchronize(stream));
    if (name == "topk_idx" || name == "keep_idx") {
        const bool tk = name == "topk_idx";
        const long n = tk ? K : max_prop;
        if (count) *count = n;
        MRCNN_REQUIRE(dst && cap >= n, MRCNN_ERR_SHAPE, "tensor '%s' needs %ld floats", name.c_str(), n);
        std::vector<int32_t> tmp((size_t)n);
        HIP_CHECK(hipMemcpy(tmp.data(), (tk ? prop_ws.topk_idx : prop_ws.keep_idx) + (size_t)image * n, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (long i = 0; i < n; ++i) dst[i] = (float)tmp[(size_t)i];
        return;
    }
    if (name == "boxes_sorted") {
        const long n = (long)K * 4;
        if (count) *count = n;
        MRCNN_REQUIRE(dst && cap >= n, MRCNN_ERR_SHAPE, "tensor '%s' needs %ld floats", name.c_str(), n);
        HIP_CHECK(hipMemcpy(dst, prop_ws.boxes + (size_t)image * n, (size_t)n * 4, hipMemcpyDeviceToHost));
        return;
    }
    if (name == "mask_row_flags") {
        const long n = max_det;
        if (count) *count = n;
        MRCNN_REQUIRE(dst && cap >= n, MRCNN_ERR_SHAPE, "tensor '%s' needs %ld floats", name.c_str(), n);
        std::vector<int32_t> tmp((size_t)n);
        HIP_CHECK(hipMemcpy(tmp.data(), msel_ws.flags + (size_t)image * n, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (long i = 0; i < n; ++i) dst[i] = (float)tmp[(size_t)i];
        return;
    }
    if (name == "keep_count") {
        if (count) *count = 1;
        MRCNN_REQUIRE(dst && cap >= 1, MRCNN_ERR_SHAPE, "tensor '%s' needs 1 float", name.c_str());
        int32_t v = 0;
        HIP_CHECK(hipMemcpy(&v, prop_ws.keep_count + image, 4, hipMemcpyDeviceToHost));
        dst[0] = (float)v;
        return;
    }
    auto it = taps.find(name);
    MRCNN_REQUIRE(it != taps.end(), MRCNN_ERR_INVALID, "unknown tensor '%s'", name.c_str());
    const long n = it->second.per_image;
    if (count) *count = n;
    MRCNN_REQUIRE(dst && cap >= n, MRCNN_ERR_SHAPE, "tensor '%s' needs %ld floats, buffer holds %lld", name.c_str(), n, (long long)cap);
    if (it->second.dtype == MRCNN_F16) {
        std::vector<uint16_t> tmp((size_t)n);
        HIP_CHECK(hipMemcpy(tmp.data(), static_cast<const uint16_t*>(it->second.base) + (size_t)image * n, (size_t)n * 2, hipMemcpyDeviceToHost));
        for (long i = 0; i < n; ++i) dst[i] = half_to_float(tmp[(size_t)i]);
    } else {
        HIP_CHECK(hipMemcpy(dst, static_cast<const float*>(it->second.base) + (size_t)image * n, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    // a tensor of a split group is stored as 2^e * value: hand out the value (exact)
    const int e = it->second.group >= 0 ? sgroups[(size_t)it->second.group].exp : 0;
    if (e != 0) for (long i = 0; i < n; ++i) dst[i] = ldexpf(dst[i], -e);
}

}  // namespace mrcnn

