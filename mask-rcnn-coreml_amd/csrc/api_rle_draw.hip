// api_rle_draw.hip — the C ABI of include/maskrcnn_hip.h, drawing run-length masks: planes, instance maps and overlays from an RLE set,
// the three host definitions (rle_draw_host.cpp behind them) and the three device entries (kernels_rle_draw.hip), which share one
// staging (RleDrawRun).  Every argument error is answered before a device is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "rle_draw_host.h"

using namespace mrcnn;

extern "C" int mrcnn_rle_decode_host(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                     const int32_t* widths, uint8_t* out, const int64_t* out_offsets)
{
    return guarded([&] {
        std::string err;
        answer(rle_draw::decode_host(rle_draw::Set{counts, run_offsets, n_images, slots, heights, widths}, out, out_offsets, &err), err);
    });
}

extern "C" int mrcnn_instance_map_rle_host(const float* detections_src, const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots,
                                           const int32_t* heights, const int32_t* widths, float min_score, int16_t* map, const int64_t* map_offsets,
                                           uint32_t* visible_areas)
{
    return guarded([&] {
        std::string err;
        answer(rle_draw::instance_map_host(rle_draw::Set{counts, run_offsets, n_images, slots, heights, widths}, detections_src, min_score, map, map_offsets,
                                           visible_areas, &err), err);
    });
}

extern "C" int mrcnn_render_detections_rle_host(const mrcnn_image* images, const float* detections_src, const uint32_t* counts,
                                                const int64_t* run_offsets, int n_images, int slots, float min_score, int alpha, int stroke,
                                                uint8_t* out_rgb, const int64_t* out_offsets)
{
    return guarded([&] {
        std::string err;
        answer(rle_draw::render_host(rle_draw::Set{counts, run_offsets, n_images, slots, nullptr, nullptr}, images, detections_src, min_score, alpha, stroke,
                                     out_rgb, out_offsets, &err), err);
    });
}

namespace {

// One call on the device.  The constructor stages what the three entries share: the RLE set on the device, its prefix table, the image
// table and the records (pass 1 of kernels_rle_draw.hip), and answers a bad RLE before anything is drawn.  The entry then draws into
// out.p, and deliver() hands the images' bytes to a host caller.
struct RleDrawRun {
    const rle_draw::Set& a;
    const char* who;
    const bool dev;
    const size_t n;
    Stream st_;
    StagedRle in;
    DevBuf td;
    Carver sc;
    RaggedOut out;                                           // (declared behind the buffers: the stream drains before they are freed)
    hipStream_t s;
    RleDrawJob job{};
    const int64_t* offsets;
    int64_t unit;

    // det: the caller's detections_src (nullptr: the decode); callers / out_offsets / unit_bytes / extent: the output and its layout, checked by the caller
    RleDrawRun(const rle_draw::Set& set, const char* name, int memspace, const float* det, float min_score, void* callers, const int64_t* out_offsets,
               int64_t unit_bytes, int64_t extent)
        : a(set), who(name), dev(memspace == MRCNN_DEVICE), n((size_t)set.n_images * set.slots), in(set.counts, set.run_offsets, (int64_t)n, dev, name),
          out(st_.s, callers, dev, extent), s(st_.s), offsets(out_offsets), unit(unit_bytes)
    {
        in.stage();
        if (!dev && det && n) det = stage_rows(det, memspace, (long)n, 6, 6, td);
        std::vector<ImageGeom> tab((size_t)a.n_images);
        for (int b = 0; b < a.n_images; ++b) {
            tab[(size_t)b].h = a.heights[b]; tab[(size_t)b].w = a.widths[b]; tab[(size_t)b].offset = offsets[b];
            job.max_h = std::max(job.max_h, a.heights[b]); job.max_w = std::max(job.max_w, a.widths[b]);
        }
        // one scratch allocation: the image table | totals | areas | extents | records | the flag
        const auto s_tab = sc.take<ImageGeom>(tab.size());
        const auto s_tot = sc.take<unsigned long long>(n);
        const auto s_ar = sc.take<uint32_t>(n);
        const auto s_ext = sc.take<uint2>(n);
        const auto s_rec = sc.take<RleDrawRec>(n);
        const auto s_bad = sc.take<unsigned long long>(1);
        sc.alloc();
        if (!tab.empty()) HIP_CHECK(hipMemcpy(sc[s_tab], tab.data(), tab.size() * sizeof(ImageGeom), hipMemcpyHostToDevice));
        job.rec = sc[s_rec];
        job.pre_b = in.pre_b;
        job.tab = sc[s_tab];
        job.n_images = a.n_images; job.slots = a.slots;
        rle_prefix_forward(s, in.counts, in.run_offsets, (long)n, in.pre_b, nullptr, sc[s_tot], sc[s_ar], sc[s_ext]);
        rle_draw_prepare(s, in.run_offsets, sc[s_tot], sc[s_ext], det, min_score, job, sc[s_rec], sc[s_bad]);
        const Refusal r = read_refusal(s, sc[s_bad], sc[s_tot]);
        std::string err;
        if (r.any) answer(rle_draw::bad_sum(a, r.k, r.sum, who, &err), err);
    }

    // the drawing is queued: only the images' own bytes go to a host caller
    void deliver(void* callers)
    {
        HIP_CHECK(hipStreamSynchronize(s));
        out.deliver(callers, offsets, a.heights, a.widths, a.n_images, unit);
    }
};

}  // namespace

extern "C" int mrcnn_rle_decode(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                const int32_t* widths, int memspace, uint8_t* out, const int64_t* out_offsets)
{
    return guarded([&] {
        std::string err;
        const rle_draw::Set a{counts, run_offsets, n_images, slots, heights, widths};
        answer(rle_draw::check_set(a, 0x7fffffff, "rle_decode", &err), err);
        MRCNN_REQUIRE(out, MRCNN_ERR_INVALID, "rle_decode: null out");
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_decode: unknown memspace %d", memspace);
        int64_t extent = 0;
        answer(check_offsets(heights, widths, n_images, out_offsets, slots, "rle_decode", &extent, &err), err);
        require_gpu();
        if (n_images == 0 || slots == 0) return;
        RleDrawRun r(a, "rle_decode", memspace, nullptr, 0.0f, out, out_offsets, slots, extent);
        rle_decode_forward(r.s, r.job, r.out.p);
        r.deliver(out);
    });
}

extern "C" int mrcnn_instance_map_rle(const float* detections_src, const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots,
                                      const int32_t* heights, const int32_t* widths, float min_score, int memspace, int16_t* map,
                                      const int64_t* map_offsets, uint32_t* visible_areas)
{
    return guarded([&] {
        std::string err;
        const rle_draw::Set a{counts, run_offsets, n_images, slots, heights, widths};
        answer(rle_draw::check_set(a, 32767, "instance_map_rle", &err), err);
        MRCNN_REQUIRE(detections_src && map, MRCNN_ERR_INVALID, "instance_map_rle: null argument");
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "instance_map_rle: unknown memspace %d", memspace);
        MRCNN_REQUIRE(reinterpret_cast<uintptr_t>(map) % 2 == 0, MRCNN_ERR_INVALID, "instance_map_rle: map is not aligned for int16");
        int64_t extent = 0;
        answer(check_offsets(heights, widths, n_images, map_offsets, 2, "instance_map_rle", &extent, &err), err);
        require_gpu();
        if (n_images == 0) return;
        RleDrawRun r(a, "instance_map_rle", memspace, detections_src, min_score, map, map_offsets, 2, extent);
        uint32_t* va = visible_areas;
        DevBuf tv;
        if (!r.dev && visible_areas) { tv.alloc(r.n * sizeof(uint32_t)); va = tv.as<uint32_t>(); }
        instance_map_rle_forward(r.s, r.job, reinterpret_cast<int16_t*>(r.out.p), va);
        r.deliver(map);
        if (!r.dev && visible_areas && r.n) HIP_CHECK(hipMemcpy(visible_areas, tv.p, r.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    });
}

extern "C" int mrcnn_render_detections_rle(const mrcnn_image* images, const float* detections_src, const uint32_t* counts, const int64_t* run_offsets,
                                           int n_images, int slots, float min_score, int alpha, int stroke, int memspace, uint8_t* out_rgb,
                                           const int64_t* out_offsets)
{
    return guarded([&] {
        std::string err;
        std::vector<int32_t> hs, ws;
        image_sizes(images, n_images, "render_detections_rle", hs, ws);
        const rle_draw::Set a{counts, run_offsets, n_images, slots, hs.data(), ws.data()};
        answer(rle_draw::check_set(a, 32767, "render_detections_rle", &err), err);
        MRCNN_REQUIRE(detections_src && out_rgb, MRCNN_ERR_INVALID, "render_detections_rle: null argument");
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "render_detections_rle: unknown memspace %d", memspace);
        answer(rle_draw::check_render(alpha, stroke, "render_detections_rle", &err), err);
        int64_t extent = 0;
        answer(check_offsets(hs.data(), ws.data(), n_images, out_offsets, 3, "render_detections_rle", &extent, &err), err);
        require_gpu();
        if (n_images == 0) return;
        RleDrawRun r(a, "render_detections_rle", memspace, detections_src, min_score, out_rgb, out_offsets, 3, extent);
        DevBuf ti, tsrc;
        tsrc.alloc((size_t)n_images * sizeof(const uint8_t*));
        upload_sources(images, n_images, r.dev, ti, tsrc.as<const uint8_t*>());
        render_detections_rle_forward(r.s, r.job, tsrc.as<const uint8_t*>(), alpha, stroke, r.out.p);
        r.deliver(out_rgb);
    });
}
