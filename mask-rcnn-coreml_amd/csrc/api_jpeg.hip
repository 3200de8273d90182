// api_jpeg.hip — the C ABI of include/maskrcnn_hip.h, JPEG: the two host entries (jpeg_host.cpp behind them) and the two device
// entries.  A batch is decoded in three steps: every header parsed and checked (nothing is written before all of them pass), the
// entropy decoders of the files on min(batch, 8) threads into ONE pinned buffer, then one upload and two launches (kernels_jpeg.hip).
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "api_util.h"
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

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

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

// steps 2 and 3: entropy decoding into sc.pinned, the upload and the two launches on `s`; image b lands at dev_out + desc[b].out_offset.
// The caller synchronises `s` before sc is used again.
void decode_on_device(const char* entry, hipStream_t s, JpegScratch& sc, const mrcnn_jpeg* files, int batch, JpegPlan& plan, uint8_t* dev_out)
{
    const size_t table_bytes = up((size_t)batch * sizeof(JpegDesc), 256), coef_bytes = (size_t)plan.total_blocks * 64 * sizeof(int16_t);
    const size_t total = table_bytes + coef_bytes;
    if (sc.pinned_bytes < total) {
        if (sc.pinned) { (void)hipHostFree(sc.pinned); sc.pinned = nullptr; sc.pinned_bytes = 0; }
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sc.pinned), total, hipHostMallocDefault));
        sc.pinned_bytes = total;
    }
    if (sc.staged.bytes < total) sc.staged.alloc(total);
    if (sc.planes.bytes < plan.plane_bytes) sc.planes.alloc(plan.plane_bytes);
    memcpy(sc.pinned, plan.desc.data(), (size_t)batch * sizeof(JpegDesc));
    int16_t* const coef = reinterpret_cast<int16_t*>(sc.pinned + table_bytes);

    std::vector<int> status((size_t)batch, MRCNN_OK);
    std::vector<std::string> errs((size_t)batch);
    std::atomic<int> next{0};
    auto work = [&] {
        for (int b = next.fetch_add(1); b < batch; b = next.fetch_add(1))
            status[(size_t)b] = jpeg::decode_coefficients(files[b].data, files[b].length, plan.hdr[(size_t)b], coef + plan.desc[(size_t)b].block0 * 64,
                                                          &errs[(size_t)b]);
    };
    const int nthreads = batch < 8 ? batch : 8;          // (never sized from the machine: a host shares its cores)
    if (nthreads == 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        pool.reserve((size_t)nthreads);
        for (int t = 0; t < nthreads; ++t) pool.emplace_back(work);
        for (std::thread& t : pool) t.join();
    }
    for (int b = 0; b < batch; ++b)
        if (status[(size_t)b] != MRCNN_OK) fail(status[(size_t)b], "%s: file %d of the batch: %s", entry, b, errs[(size_t)b].c_str());

    HIP_CHECK(hipMemcpyAsync(sc.staged.p, sc.pinned, total, hipMemcpyHostToDevice, s));
    jpeg_decode_forward(s, sc.staged.as<JpegDesc>(), batch, reinterpret_cast<const int16_t*>(sc.staged.as<uint8_t>() + table_bytes), plan.total_blocks,
                        sc.planes.as<uint8_t>(), plan.total_chunks, dev_out);
}

// mrcnn_jpeg_decode_batch has no handle to keep its staging in: one per process, handed to one call at a time.  Never freed — at
// process exit the HIP runtime may be gone before a static destructor would run.
JpegScratch& shared_scratch() { static JpegScratch* sc = new JpegScratch; return *sc; }
std::mutex g_scratch_mutex;

}  // namespace

extern "C" int mrcnn_jpeg_decode_batch(const mrcnn_jpeg* files, int batch, int memspace, uint8_t* out_rgb, const int64_t* out_offsets,
                                       int32_t* heights, int32_t* widths)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(files && out_rgb && out_offsets && heights && widths, MRCNN_ERR_INVALID, "null jpeg_decode_batch argument");
        MRCNN_REQUIRE(batch >= 1 && batch <= MRCNN_JPEG_MAX_BATCH, MRCNN_ERR_SHAPE, "jpeg_decode_batch: batch %d outside 1..%d", batch, MRCNN_JPEG_MAX_BATCH);
        const auto t0 = std::chrono::steady_clock::now();
        JpegPlan plan;
        plan_batch("jpeg_decode_batch", files, batch, plan);
        int64_t extent = 0;
        auto bytes_of = [&](int b) { return (int64_t)3 * plan.desc[(size_t)b].h * plan.desc[(size_t)b].w; };
        for (int b = 0; b < batch; ++b) {
            const int64_t off = out_offsets[b];
            MRCNN_REQUIRE(off >= 0 && off % 16 == 0, MRCNN_ERR_INVALID, "jpeg_decode_batch: file %d of the batch: out_offsets[%d] = %lld is not a non-negative multiple of 16",
                          b, b, (long long)off);
            plan.desc[(size_t)b].out_offset = off;
            extent = off + bytes_of(b) > extent ? off + bytes_of(b) : extent;
        }
        for (int a = 0; a < batch; ++a)
            for (int b = a + 1; b < batch; ++b) {
                const int64_t a0 = out_offsets[a], a1 = a0 + bytes_of(a), b0 = out_offsets[b], b1 = b0 + bytes_of(b);
                MRCNN_REQUIRE(a1 <= b0 || b1 <= a0, MRCNN_ERR_INVALID, "jpeg_decode_batch: files %d and %d overlap in the output", a, b);
            }
        for (int b = 0; b < batch; ++b) { heights[b] = plan.desc[(size_t)b].h; widths[b] = plan.desc[(size_t)b].w; }
        const bool dev = memspace == MRCNN_DEVICE;
        std::lock_guard<std::mutex> lock(g_scratch_mutex);
        JpegScratch& sc = shared_scratch();
        Stream st;
        uint8_t* o = out_rgb;
        if (!dev) {             // (same offsets as the caller's buffer: only the images are copied back)
            if (sc.rgb.bytes < (size_t)extent) sc.rgb.alloc((size_t)extent);
            o = sc.rgb.as<uint8_t>();
        }
        struct Drain {          // an error after the upload was queued must not leave it reading the staging the next call rewrites
            hipStream_t s;
            ~Drain() { (void)hipStreamSynchronize(s); }
        } drain{st.s};
        decode_on_device("jpeg_decode_batch", st.s, sc, files, batch, plan, o);
        t_host_ms = (float)ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        HIP_CHECK(hipStreamSynchronize(st.s));
        t_device_ms = (float)ms_since(t1);
        if (!dev)
            for (int b = 0; b < batch; ++b)
                HIP_CHECK(hipMemcpy(out_rgb + out_offsets[b], o + out_offsets[b], (size_t)bytes_of(b), hipMemcpyDeviceToHost));
    });
}

extern "C" int mrcnn_maskrcnn_predict_jpegs(mrcnn_model* model, const mrcnn_jpeg* files, int batch, int memspace, float* detections,
                                            float* masks, int32_t* heights, int32_t* widths)
{
    (void)memspace;             // (the record copies follow the pointers, as in predict_images)
    return guarded([&] {
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
        struct Drain {
            hipStream_t s;
            ~Drain() { (void)hipStreamSynchronize(s); }
        } drain{m.stream};
        decode_on_device("predict_jpegs", m.stream, sc, files, batch, plan, sc.rgb.as<uint8_t>());
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
