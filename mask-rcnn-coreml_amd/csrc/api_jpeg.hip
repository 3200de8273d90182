// api_jpeg.hip — the C ABI of include/maskrcnn_hip.h, JPEG: the two host entries (jpeg_host.cpp behind them) and the two device
// entries.  A batch is decoded in three steps: every header parsed and checked (nothing is written before all of them pass), the
// entropy decoders of the files on min(batch, 8) threads into ONE pinned buffer, then one upload and two launches (kernels_jpeg.hip).
// With MRCNN_JPEG_ENTROPY_DEVICE the second step runs on the device instead (kernels_jpeg_entropy.hip): the files' bytes are uploaded,
// and only the files its verdict does not call clean go through the host decoder, whose answer is then the call's.
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "api_util.h"
#include "jpeg_entropy_host.h"
#include "kernels_jpeg_entropy.h"
#include "jpeg_host.h"

using namespace mrcnn;

extern "C" int mrcnn_jpeg_info(const uint8_t* data, int64_t length, int32_t* height, int32_t* width, int32_t* components, int32_t* h_samp,
                               int32_t* v_samp)
{
    return guarded([&] {
        MRCNN_REQUIRE((data || length == 0) && length >= 0, MRCNN_ERR_INVALID, "jpeg_info: null data or negative length");
        jpeg::Header h;
        std::string err;
        const int st = jpeg::parse(data, length, &h, &err);
        if (st != MRCNN_OK) fail(st, "%s", err.c_str());
        if (height) *height = h.height;
        if (width) *width = h.width;
        if (components) *components = h.components;
        if (h_samp) *h_samp = h.h_samp;
        if (v_samp) *v_samp = h.v_samp;
    });
}

extern "C" int mrcnn_jpeg_decode_host(const uint8_t* data, int64_t length, uint8_t* rgb, int64_t capacity)
{
    return guarded([&] {
        MRCNN_REQUIRE((data || length == 0) && length >= 0 && rgb && capacity >= 0, MRCNN_ERR_INVALID, "jpeg_decode_host: null buffer or negative size");
        std::string err;
        const int st = jpeg::decode_host(data, length, rgb, capacity, &err);
        if (st != MRCNN_OK) fail(st, "%s", err.c_str());
    });
}

namespace {

thread_local float t_host_ms = 0, t_device_ms = 0;
double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct JpegPlan {
    std::vector<jpeg::Header> hdr;
    std::vector<JpegDesc> desc;
    long long total_blocks = 0, total_chunks = 0;
    size_t plane_bytes = 0;
};

// step 1: every file parsed and checked against the decoder's scope; the layout of the batch on the device
void plan_batch(const char* entry, const mrcnn_jpeg* files, int batch, JpegPlan& plan)
{
    plan.hdr.resize((size_t)batch);
    plan.desc.resize((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        MRCNN_REQUIRE(files[b].data && files[b].length > 0, MRCNN_ERR_INVALID, "%s: file %d of the batch: null data or no bytes", entry, b);
        jpeg::Header& h = plan.hdr[(size_t)b];
        std::string err;
        const int st = jpeg::parse(files[b].data, files[b].length, &h, &err);
        if (st != MRCNN_OK) fail(st, "%s: file %d of the batch: %s", entry, b, err.c_str());
        JpegDesc& d = plan.desc[(size_t)b];
        memset(&d, 0, sizeof d);
        d.h = h.height; d.w = h.width; d.ncomp = h.components; d.mode = h.mode;
        d.block0 = plan.total_blocks;
        d.chunk0 = plan.total_chunks;
        for (int c = 0; c < h.components; ++c) {
            const jpeg::Component& k = h.comp[c];
            JpegComp& o = d.comp[c];
            o.block0 = plan.total_blocks + k.block0;
            o.plane0 = (long long)plan.plane_bytes;
            o.blocks_w = k.blocks_w; o.blocks_h = k.blocks_h; o.width = k.width; o.height = k.height;
            plan.plane_bytes += up((size_t)k.blocks_w * k.blocks_h * 64, 16);
            memcpy(d.quant[c], h.quant[k.tq], sizeof d.quant[c]);
        }
        plan.total_blocks += h.total_blocks;
        plan.total_chunks += ((long long)h.height * h.width + 15) / 16;
    }
}

void grow_pinned(JpegScratch& sc, size_t total)
{
    if (sc.pinned_bytes < total) {
        if (sc.pinned) { (void)hipHostFree(sc.pinned); sc.pinned = nullptr; sc.pinned_bytes = 0; }
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sc.pinned), total, hipHostMallocDefault));
        sc.pinned_bytes = total;
    }
}

// the host decoder over files `which` of the batch on min(count, 8) threads, file b into coef_of(b); the first failure in batch order
// is the call's, in the wording every entry shares
template <class CoefOf> void decode_on_host(const char* entry, const mrcnn_jpeg* files, const JpegPlan& plan, const std::vector<int>& which, CoefOf coef_of)
{
    const int count = (int)which.size();
    std::vector<int> status((size_t)count, MRCNN_OK);
    std::vector<std::string> errs((size_t)count);
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i = next.fetch_add(1); i < count; i = next.fetch_add(1)) {
            const int b = which[(size_t)i];
            status[(size_t)i] = jpeg::decode_coefficients(files[b].data, files[b].length, plan.hdr[(size_t)b], coef_of(b), &errs[(size_t)i]);
        }
    };
    const int nthreads = count < 8 ? count : 8;          // (never sized from the machine: a host shares its cores)
    if (nthreads <= 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        pool.reserve((size_t)nthreads);
        for (int t = 0; t < nthreads; ++t) pool.emplace_back(work);
        for (std::thread& t : pool) t.join();
    }
    for (int i = 0; i < count; ++i)
        if (status[(size_t)i] != MRCNN_OK) fail(status[(size_t)i], "%s: file %d of the batch: %s", entry, which[(size_t)i], errs[(size_t)i].c_str());
}

// every file of the batch through the host decoder, file b to its place in the batch's coefficient array at `coef`
void decode_all_on_host(const char* entry, const mrcnn_jpeg* files, const JpegPlan& plan, int16_t* coef)
{
    std::vector<int> all(plan.desc.size());
    for (size_t b = 0; b < all.size(); ++b) all[b] = (int)b;
    decode_on_host(entry, files, plan, all, [&](int b) { return coef + plan.desc[(size_t)b].block0 * 64; });
}

// the marker scan of the batch (jpeg_entropy_host.h), for the device stage and for its host model
jpeg::EntropyPlan entropy_plan(const mrcnn_jpeg* files, int batch, const JpegPlan& plan, int unit_bytes)
{
    std::vector<long long> block0((size_t)batch);
    for (int b = 0; b < batch; ++b) block0[(size_t)b] = plan.desc[(size_t)b].block0;
    jpeg::EntropyPlan ep;
    jpeg::plan_entropy(files, plan.hdr.data(), block0.data(), batch, unit_bytes, ep);
    return ep;
}

// the knobs of mrcnn_jpeg_coefficients (0 = production) and what it reports
struct EntropyKnobs {
    int unit_bytes = 0, max_rounds = 0;
    int clean = 0, fell_back = 0, rounds = 0, units = 0;
};

// Step 2 on the device.  Uploads the descriptor table, the plan of the marker scan and the files' BYTES, runs the entropy launches into
// the coefficient array behind them in sc.staged, reads the verdict words back (one copy, one synchronisation) and gives every file that
// is not clean to the host decoder, whose coefficients are uploaded over the device's.  Returns the offset of the coefficients in sc.staged.
size_t entropy_on_device(const char* entry, hipStream_t s, JpegScratch& sc, const mrcnn_jpeg* files, int batch, JpegPlan& plan, EntropyKnobs& knobs)
{
    const jpeg::EntropyPlan ep = entropy_plan(files, batch, plan, knobs.unit_bytes);
    const int nsegs = (int)ep.segs.size(), nunits = (int)ep.unit_seg.size(), nwg = (int)ep.wgs.size();
    // the upload: descriptors | files | segments | unit -> segment | workgroups | bytes ; behind it on the device: the coefficients
    const size_t o_files = up((size_t)batch * sizeof(JpegDesc), 256), o_segs = o_files + up((size_t)batch * sizeof(jpeg::EntFile), 256),
                 o_unit = o_segs + up((size_t)nsegs * sizeof(jpeg::EntSeg), 256), o_wgs = o_unit + up((size_t)nunits * sizeof(int32_t), 256),
                 o_bytes = o_wgs + up((size_t)nwg * sizeof(jpeg::EntWg), 256), upload = o_bytes + up((size_t)ep.blob_bytes, 256);
    const size_t coef_bytes = (size_t)plan.total_blocks * 64 * sizeof(int16_t), verdict_bytes = ((size_t)2 * batch + 1) * sizeof(int32_t);
    const size_t o_verdict_host = upload;                 // (pinned only: where the verdict words come back)
    grow_pinned(sc, upload + up(verdict_bytes, 256));
    if (sc.staged.bytes < upload + coef_bytes) sc.staged.alloc(upload + coef_bytes);
    if (sc.planes.bytes < plan.plane_bytes) sc.planes.alloc(plan.plane_bytes);
    memcpy(sc.pinned, plan.desc.data(), (size_t)batch * sizeof(JpegDesc));
    memcpy(sc.pinned + o_files, ep.files.data(), (size_t)batch * sizeof(jpeg::EntFile));
    if (nsegs) memcpy(sc.pinned + o_segs, ep.segs.data(), (size_t)nsegs * sizeof(jpeg::EntSeg));
    if (nunits) memcpy(sc.pinned + o_unit, ep.unit_seg.data(), (size_t)nunits * sizeof(int32_t));
    if (nwg) memcpy(sc.pinned + o_wgs, ep.wgs.data(), (size_t)nwg * sizeof(jpeg::EntWg));
    for (int b = 0; b < batch; ++b) memcpy(sc.pinned + o_bytes + ep.files[(size_t)b].byte0, files[b].data, (size_t)files[b].length);
    // the launches' own words: all ones (no state yet) | zeros
    const size_t ones = ((size_t)nunits + 3 * (size_t)nwg) * 8, zeros = ((size_t)2 * nunits + 1 + 2 * (size_t)nwg + 2 * (size_t)batch + 1) * 4;
    if (sc.ent_work.bytes < ones + zeros) sc.ent_work.alloc(ones + zeros);
    uint8_t* const dev = sc.staged.as<uint8_t>();
    uint8_t* const wk = sc.ent_work.as<uint8_t>();
    JpegEntBuffers eb;
    eb.files = reinterpret_cast<const jpeg::EntFile*>(dev + o_files);
    eb.segs = reinterpret_cast<const jpeg::EntSeg*>(dev + o_segs);
    eb.unit_seg = reinterpret_cast<const int32_t*>(dev + o_unit);
    eb.wgs = reinterpret_cast<const jpeg::EntWg*>(dev + o_wgs);
    eb.bytes = dev + o_bytes;
    eb.state = reinterpret_cast<unsigned long long*>(wk);
    eb.wg_exit = eb.state + nunits;
    eb.wg_entry = eb.wg_exit + 2 * (size_t)nwg;
    eb.count = reinterpret_cast<uint32_t*>(wk + ones);
    eb.prefix = eb.count + nunits;
    eb.wg_flags = reinterpret_cast<int32_t*>(eb.prefix + nunits + 1);
    eb.verdict = eb.wg_flags + 2 * (size_t)nwg;
    eb.batch = batch; eb.nsegs = nsegs; eb.nunits = nunits; eb.nwg = nwg; eb.unit_bytes = ep.unit_bytes;
    eb.launches = jpeg::ent_launches(ep.unit_bytes, ep.max_file_wgs, knobs.max_rounds);
    eb.inner_rounds = jpeg::ent_inner_rounds(knobs.max_rounds);
    int16_t* const dcoef = reinterpret_cast<int16_t*>(dev + upload);
    HIP_CHECK(hipMemcpyAsync(dev, sc.pinned, upload, hipMemcpyHostToDevice, s));
    if (ones) HIP_CHECK(hipMemsetAsync(wk, 0xFF, ones, s));
    HIP_CHECK(hipMemsetAsync(wk + ones, 0, zeros, s));
    jpeg_entropy_forward(s, eb, dcoef, plan.total_blocks);
    int32_t* const verdict = reinterpret_cast<int32_t*>(sc.pinned + o_verdict_host);
    HIP_CHECK(hipMemcpyAsync(verdict, eb.verdict, verdict_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int> fallback;
    for (int b = 0; b < batch; ++b)
        if (!jpeg::ent_clean(ep.files[(size_t)b], verdict[2 * b], verdict[2 * b + 1], eb.launches)) fallback.push_back(b);
    knobs.clean = batch - (int)fallback.size(); knobs.fell_back = (int)fallback.size(); knobs.rounds = verdict[2 * batch]; knobs.units = nunits;
    if (!fallback.empty()) {
        std::vector<std::vector<int16_t>> host_coef((size_t)batch);
        for (int b : fallback) host_coef[(size_t)b].resize((size_t)plan.hdr[(size_t)b].total_blocks * 64);
        decode_on_host(entry, files, plan, fallback, [&](int b) { return host_coef[(size_t)b].data(); });
        for (int b : fallback)
            HIP_CHECK(hipMemcpyAsync(dcoef + plan.desc[(size_t)b].block0 * 64, host_coef[(size_t)b].data(), host_coef[(size_t)b].size() * sizeof(int16_t),
                                     hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));             // (host_coef is pageable and goes out of scope)
    }
    return upload;
}

// steps 2 and 3: entropy decoding (on the host into sc.pinned and one upload, or on the device), then the two launches on `s`; image b
// lands at dev_out + desc[b].out_offset.  The caller synchronises `s` before sc is used again.
void decode_on_device(const char* entry, hipStream_t s, JpegScratch& sc, const mrcnn_jpeg* files, int batch, JpegPlan& plan, int entropy, uint8_t* dev_out)
{
    if (entropy == MRCNN_JPEG_ENTROPY_DEVICE) {
        EntropyKnobs knobs;
        const size_t o_coef = entropy_on_device(entry, s, sc, files, batch, plan, knobs);
        jpeg_decode_forward(s, sc.staged.as<JpegDesc>(), batch, reinterpret_cast<const int16_t*>(sc.staged.as<uint8_t>() + o_coef), plan.total_blocks,
                            sc.planes.as<uint8_t>(), plan.total_chunks, dev_out);
        return;
    }
    const size_t table_bytes = up((size_t)batch * sizeof(JpegDesc), 256), coef_bytes = (size_t)plan.total_blocks * 64 * sizeof(int16_t);
    const size_t total = table_bytes + coef_bytes;
    grow_pinned(sc, total);
    if (sc.staged.bytes < total) sc.staged.alloc(total);
    if (sc.planes.bytes < plan.plane_bytes) sc.planes.alloc(plan.plane_bytes);
    memcpy(sc.pinned, plan.desc.data(), (size_t)batch * sizeof(JpegDesc));
    decode_all_on_host(entry, files, plan, reinterpret_cast<int16_t*>(sc.pinned + table_bytes));

    HIP_CHECK(hipMemcpyAsync(sc.staged.p, sc.pinned, total, hipMemcpyHostToDevice, s));
    jpeg_decode_forward(s, sc.staged.as<JpegDesc>(), batch, reinterpret_cast<const int16_t*>(sc.staged.as<uint8_t>() + table_bytes), plan.total_blocks,
                        sc.planes.as<uint8_t>(), plan.total_chunks, dev_out);
}

void require_entropy(const char* entry, int entropy)
{
    MRCNN_REQUIRE(entropy == MRCNN_JPEG_ENTROPY_HOST || entropy == MRCNN_JPEG_ENTROPY_DEVICE, MRCNN_ERR_INVALID,
                  "%s: entropy %d is neither MRCNN_JPEG_ENTROPY_HOST (0) nor MRCNN_JPEG_ENTROPY_DEVICE (1)", entry, entropy);
}

// mrcnn_jpeg_decode_batch has no handle to keep its staging in: one per process, handed to one call at a time.  Never freed — at
// process exit the HIP runtime may be gone before a static destructor would run.
JpegScratch& shared_scratch() { static JpegScratch* sc = new JpegScratch; return *sc; }
std::mutex g_scratch_mutex;

}  // namespace

extern "C" int mrcnn_jpeg_decode_batch(const mrcnn_jpeg* files, int batch, int memspace, uint8_t* out_rgb, const int64_t* out_offsets,
                                       int32_t* heights, int32_t* widths)
{
    return mrcnn_jpeg_decode_batch_on(files, batch, memspace, MRCNN_JPEG_ENTROPY_HOST, out_rgb, out_offsets, heights, widths);
}

extern "C" int mrcnn_jpeg_decode_batch_on(const mrcnn_jpeg* files, int batch, int memspace, int entropy, uint8_t* out_rgb, const int64_t* out_offsets,
                                          int32_t* heights, int32_t* widths)
{
    return guarded([&] {
        require_entropy("jpeg_decode_batch", entropy);
        require_gpu();
        MRCNN_REQUIRE(files && out_rgb && out_offsets && heights && widths, MRCNN_ERR_INVALID, "null jpeg_decode_batch argument");
        MRCNN_REQUIRE(batch >= 1 && batch <= MRCNN_JPEG_MAX_BATCH, MRCNN_ERR_SHAPE, "jpeg_decode_batch: batch %d outside 1..%d", batch, MRCNN_JPEG_MAX_BATCH);
        const auto t0 = std::chrono::steady_clock::now();
        JpegPlan plan;
        plan_batch("jpeg_decode_batch", files, batch, plan);
        std::vector<int32_t> hs((size_t)batch), ws((size_t)batch);
        for (int b = 0; b < batch; ++b) { hs[(size_t)b] = plan.desc[(size_t)b].h; ws[(size_t)b] = plan.desc[(size_t)b].w; }
        int64_t extent = 0;
        std::string err;
        answer(check_offsets(hs.data(), ws.data(), batch, out_offsets, 3, "jpeg_decode_batch", &extent, &err), err);
        for (int b = 0; b < batch; ++b) { plan.desc[(size_t)b].out_offset = out_offsets[b]; heights[b] = hs[(size_t)b]; widths[b] = ws[(size_t)b]; }
        const bool dev = memspace == MRCNN_DEVICE;
        std::lock_guard<std::mutex> lock(g_scratch_mutex);
        JpegScratch& sc = shared_scratch();
        Stream st;
        uint8_t* o = out_rgb;
        if (!dev) {             // (same offsets as the caller's buffer: only the images are copied back)
            if (sc.rgb.bytes < (size_t)extent) sc.rgb.alloc((size_t)extent);
            o = sc.rgb.as<uint8_t>();
        }
        Drain drain{st.s};
        decode_on_device("jpeg_decode_batch", st.s, sc, files, batch, plan, entropy, o);
        t_host_ms = (float)ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        HIP_CHECK(hipStreamSynchronize(st.s));
        t_device_ms = (float)ms_since(t1);
        if (!dev) ragged_to_host(out_rgb, o, out_offsets, hs.data(), ws.data(), batch, 3);
    });
}

extern "C" int mrcnn_maskrcnn_predict_jpegs(mrcnn_model* model, const mrcnn_jpeg* files, int batch, int memspace, float* detections,
                                            float* masks, int32_t* heights, int32_t* widths)
{
    return mrcnn_maskrcnn_predict_jpegs_on(model, files, batch, memspace, MRCNN_JPEG_ENTROPY_HOST, detections, masks, heights, widths);
}

extern "C" int mrcnn_maskrcnn_predict_jpegs_on(mrcnn_model* model, const mrcnn_jpeg* files, int batch, int memspace, int entropy, float* detections,
                                               float* masks, int32_t* heights, int32_t* widths)
{
    (void)memspace;             // (the record copies follow the pointers, as in predict_images)
    return guarded([&] {
        require_entropy("predict_jpegs", entropy);
        require_gpu();
        MRCNN_REQUIRE(model && files && detections && masks && heights && widths, MRCNN_ERR_INVALID, "null predict_jpegs argument");
        Model& m = model->m;
        MRCNN_REQUIRE(m.kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "predict_jpegs called on a non-MaskRCNN model");
        MRCNN_REQUIRE(batch >= 1 && batch <= m.max_batch, MRCNN_ERR_SHAPE, "batch %d outside 1..%d", batch, m.max_batch);
        const auto t0 = std::chrono::steady_clock::now();
        JpegPlan plan;
        plan_batch("predict_jpegs", files, batch, plan);
        size_t total = 0;
        for (int b = 0; b < batch; ++b) {
            JpegDesc& d = plan.desc[(size_t)b];
            d.out_offset = (long long)total;
            total += up((size_t)3 * d.h * d.w, 16);
            heights[b] = d.h; widths[b] = d.w;
        }
        JpegScratch& sc = m.jpeg;
        if (sc.rgb.bytes < total) { HIP_CHECK(hipStreamSynchronize(m.stream)); sc.rgb.alloc(total); }
        Drain drain{m.stream};
        decode_on_device("predict_jpegs", m.stream, sc, files, batch, plan, entropy, sc.rgb.as<uint8_t>());
        t_host_ms = (float)ms_since(t0);
        t_device_ms = 0;
        // the decoded images never leave the device: predict_images takes them as any caller's device images, on the same stream
        std::vector<mrcnn_image> images((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            const JpegDesc& d = plan.desc[(size_t)b];
            images[(size_t)b].rgb = sc.rgb.as<uint8_t>() + d.out_offset;
            images[(size_t)b].height = d.h;
            images[(size_t)b].width = d.w;
        }
        m.predict_images(images.data(), batch, MRCNN_DEVICE, detections, masks);
    });
}

extern "C" int mrcnn_jpeg_last_stage_ms(float* host_ms, float* device_ms)
{
    return guarded([&] {
        MRCNN_REQUIRE(host_ms && device_ms, MRCNN_ERR_INVALID, "null jpeg_last_stage_ms argument");
        *host_ms = t_host_ms;
        *device_ms = t_device_ms;
    });
}

// Test entry (include/maskrcnn_hip_test.h): the coefficients of a batch from the host decoder, the device stage or the host model
extern "C" int mrcnn_jpeg_coefficients(const mrcnn_jpeg* files, int batch, int entropy, int unit_bytes, int max_rounds, int16_t* coef, int64_t capacity,
                                       int64_t* block0, int32_t* stats)
{
    return guarded([&] {
        MRCNN_REQUIRE(files && block0 && stats && (coef || capacity == 0) && capacity >= 0, MRCNN_ERR_INVALID, "null jpeg_coefficients argument");
        MRCNN_REQUIRE(entropy >= 0 && entropy <= 2, MRCNN_ERR_INVALID, "jpeg_coefficients: entropy %d outside 0 (host), 1 (device), 2 (host model)", entropy);
        MRCNN_REQUIRE(unit_bytes == 0 || (unit_bytes >= 4 && unit_bytes <= 1024 && (unit_bytes & (unit_bytes - 1)) == 0), MRCNN_ERR_INVALID,
                      "jpeg_coefficients: unit_bytes %d is neither 0 nor a power of two in 4..1024", unit_bytes);
        MRCNN_REQUIRE(max_rounds >= 0, MRCNN_ERR_INVALID, "jpeg_coefficients: max_rounds %d is negative", max_rounds);
        MRCNN_REQUIRE((unit_bytes == 0 && max_rounds == 0) || test_knobs_armed(), MRCNN_ERR_UNSUPPORTED,
                      "jpeg_coefficients: unit_bytes and max_rounds are armed only in a process started with MRCNN_TEST_KNOBS=1 (include/maskrcnn_hip_test.h)");
        MRCNN_REQUIRE(batch >= 1 && batch <= MRCNN_JPEG_MAX_BATCH, MRCNN_ERR_SHAPE, "jpeg_coefficients: batch %d outside 1..%d", batch, MRCNN_JPEG_MAX_BATCH);
        if (entropy == MRCNN_JPEG_ENTROPY_DEVICE) require_gpu();
        JpegPlan plan;
        plan_batch("jpeg_coefficients", files, batch, plan);
        for (int b = 0; b < batch; ++b) block0[b] = plan.desc[(size_t)b].block0;
        block0[batch] = plan.total_blocks;
        MRCNN_REQUIRE(capacity >= plan.total_blocks * 64, MRCNN_ERR_SHAPE, "jpeg_coefficients: the batch holds %lld coefficients, the buffer %lld",
                      plan.total_blocks * 64, (long long)capacity);
        EntropyKnobs knobs;
        knobs.unit_bytes = unit_bytes; knobs.max_rounds = max_rounds;
        if (entropy == MRCNN_JPEG_ENTROPY_HOST) {
            decode_all_on_host("jpeg_coefficients", files, plan, coef);
        } else if (entropy == MRCNN_JPEG_ENTROPY_DEVICE) {
            std::lock_guard<std::mutex> lock(g_scratch_mutex);
            JpegScratch& sc = shared_scratch();
            Stream st;
            Drain drain{st.s};
            const size_t o_coef = entropy_on_device("jpeg_coefficients", st.s, sc, files, batch, plan, knobs);
            HIP_CHECK(hipMemcpyAsync(coef, sc.staged.as<uint8_t>() + o_coef, (size_t)plan.total_blocks * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, st.s));
            HIP_CHECK(hipStreamSynchronize(st.s));
        } else {
            const jpeg::EntropyPlan ep = entropy_plan(files, batch, plan, unit_bytes);
            std::vector<char> clean;
            jpeg::entropy_model(ep, files, max_rounds, coef, plan.total_blocks, clean, &knobs.rounds);
            std::vector<int> fallback;
            for (int b = 0; b < batch; ++b)
                if (!clean[(size_t)b]) fallback.push_back(b);
            knobs.clean = batch - (int)fallback.size(); knobs.fell_back = (int)fallback.size(); knobs.units = (int)ep.unit_seg.size();
            decode_on_host("jpeg_coefficients", files, plan, fallback, [&](int b) { return coef + plan.desc[(size_t)b].block0 * 64; });
        }
        stats[0] = knobs.clean; stats[1] = knobs.fell_back; stats[2] = knobs.rounds; stats[3] = knobs.units;
    });
}
