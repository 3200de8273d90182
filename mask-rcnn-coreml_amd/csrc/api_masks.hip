// api_masks.hip — the C ABI of include/maskrcnn_hip.h, masks in image pixels: paste into planes, COCO run-length
// encoding on the GPU and COCO's compressed RLE string.
#include "api_util.h"

using namespace mrcnn;

// ================================================================================================
// mask paste (DetectionRenderer.swift:13-24)
// ================================================================================================
extern "C" int mrcnn_paste_masks(const float* detections, int64_t det_stride, const float* masks, int n, int mask_size, int image_h,
                                 int image_w, float threshold, int memspace, uint8_t* out)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(detections && masks && out && n >= 0 && det_stride >= 6 && mask_size >= 2 && image_h > 0 && image_w > 0,
                      MRCNN_ERR_INVALID, "bad paste_masks argument");
        if (n == 0) return;
        Stream st;
        DevBuf td, tm, to;
        Drain drain{st.s};
        const float* d = stage_rows(detections, memspace, n, det_stride, det_stride, td);
        const float* m = stage_rows(masks, memspace, n, (long)mask_size * mask_size, (long)mask_size * mask_size, tm);
        uint8_t* o = out;
        const size_t bytes = (size_t)n * image_h * image_w;
        if (memspace != MRCNN_DEVICE) { to.alloc(bytes); o = to.as<uint8_t>(); }
        paste_masks_forward(st.s, d, det_stride, m, n, mask_size, image_h, image_w, threshold, o);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (memspace != MRCNN_DEVICE) HIP_CHECK(hipMemcpy(out, to.p, bytes, hipMemcpyDeviceToHost));
    });
}

// the geometry table of a mixed-size batch: every image's size checked (ragged.h), its letterbox at the model's input size, and its place
// in a ragged output of `unit` bytes per pixel (offsets == nullptr: no such output, offset 0), checked too.  *extent = the output's
// end, *max_pixels = the largest h*w.
static std::vector<ImageGeom> image_geometry(const char* who, const int32_t* heights, const int32_t* widths, int batch, int model_h, int model_w,
                                             const int64_t* offsets = nullptr, int64_t unit = 0, int64_t* extent = nullptr, long* max_pixels = nullptr)
{
    std::string err;
    answer(check_sides(heights, widths, batch, who, &err), err);
    if (offsets) answer(check_offsets(heights, widths, batch, offsets, unit, who, extent, &err), err);
    std::vector<ImageGeom> geom((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        ImageGeom& g = geom[(size_t)b];
        g.h = heights[b]; g.w = widths[b]; g.offset = offsets ? offsets[b] : 0; g.pitch = g.w;
        MRCNN_REQUIRE(mrcnn_letterbox_geometry(g.h, g.w, model_h, model_w, &g.nh, &g.nw, &g.py, &g.px) == MRCNN_OK, MRCNN_ERR_INVALID,
                      "%s: image %d: bad letterbox geometry", who, b);
        if (max_pixels) *max_pixels = std::max(*max_pixels, (long)g.h * g.w);
    }
    return geom;
}

extern "C" int mrcnn_paste_masks_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                        const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                        int memspace, float* detections_src, uint8_t* out, const int64_t* out_offsets)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(detections && masks && heights && widths && detections_src && out && out_offsets, MRCNN_ERR_INVALID, "null paste_masks_source argument");
        MRCNN_REQUIRE(batch >= 0 && rows >= 0 && mask_size >= 2 && model_h > 0 && model_w > 0, MRCNN_ERR_INVALID, "bad paste_masks_source argument");
        MRCNN_REQUIRE((long)batch * rows < (1L << 31), MRCNN_ERR_SHAPE, "paste_masks_source: %d x %d rows are too many", batch, rows);
        if (batch == 0 || rows == 0) return;
        int64_t extent = 0;
        long max_pixels = 0;
        const std::vector<ImageGeom> geom = image_geometry("paste_masks_source", heights, widths, batch, model_h, model_w, out_offsets, rows, &extent, &max_pixels);
        const bool dev = memspace == MRCNN_DEVICE;
        Stream st;
        DevBuf td, tm, ts;
        const size_t n = (size_t)batch * rows;
        const float* d = stage_rows(detections, memspace, (long)n, 6, 6, td);
        const float* m = stage_rows(masks, memspace, (long)n, (long)mask_size * mask_size, (long)mask_size * mask_size, tm);
        float* ds = detections_src;
        if (!dev) { ts.alloc(n * 6 * sizeof(float)); ds = ts.as<float>(); }
        Carver sc;                                              // one scratch allocation: the geometry table | the pixel boxes
        const auto tab = sc.take<ImageGeom>((size_t)batch);
        const auto box = sc.take<int4>(n);
        sc.alloc();
        RaggedOut o(st.s, out, dev, extent);
        HIP_CHECK(hipMemcpy(sc[tab], geom.data(), (size_t)batch * sizeof(ImageGeom), hipMemcpyHostToDevice));
        paste_masks_source_forward(st.s, d, m, sc[tab], batch, rows, mask_size, model_h, model_w, rows * max_pixels, threshold, ds, sc[box], o.p);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) HIP_CHECK(hipMemcpy(detections_src, ts.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost));
        o.deliver(out, out_offsets, heights, widths, batch, rows);
    });
}

// COCO run-length encoding of the masks mrcnn_paste_masks_source would paste: two steps with the capacity check between them
extern "C" int mrcnn_masks_rle_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                      const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                      int memspace, float* detections_src, uint32_t* counts, int64_t capacity, int64_t* run_offsets,
                                      uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(detections && masks && heights && widths && detections_src && run_offsets, MRCNN_ERR_INVALID, "null masks_rle_source argument");
        MRCNN_REQUIRE(capacity >= 0 && (counts || capacity == 0), MRCNN_ERR_INVALID, "masks_rle_source: null counts with capacity %lld", (long long)capacity);
        MRCNN_REQUIRE(batch >= 0 && rows >= 0 && mask_size >= 2 && model_h > 0 && model_w > 0, MRCNN_ERR_INVALID, "bad masks_rle_source argument");
        MRCNN_REQUIRE((long)batch * rows < (1L << 31), MRCNN_ERR_SHAPE, "masks_rle_source: %d x %d rows are too many", batch, rows);
        const std::vector<ImageGeom> geom = image_geometry("masks_rle_source", heights, widths, batch, model_h, model_w);
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t n = (size_t)batch * rows;
        Stream st;
        DevBuf td, tm, ts, to, ta, tx, tc;
        Carver sc;                                              // one scratch allocation: the geometry table | the pixel boxes | the segment records | the runs per instance
        Drain drain{st.s};
        const float* d = stage_rows(detections, memspace, (long)n, 6, 6, td);
        const float* m = stage_rows(masks, memspace, (long)n, (long)mask_size * mask_size, (long)mask_size * mask_size, tm);
        float* ds = detections_src;
        long long* ro = reinterpret_cast<long long*>(run_offsets);
        uint32_t* ar = areas;
        int32_t* bb = bboxes_xywh;
        if (!dev) {
            ts.alloc(n * 6 * sizeof(float)); ds = ts.as<float>();
            to.alloc((n + 1) * sizeof(long long)); ro = to.as<long long>();
            if (areas) { ta.alloc(n * sizeof(uint32_t)); ar = ta.as<uint32_t>(); }
            if (bboxes_xywh) { tx.alloc(n * 4 * sizeof(int32_t)); bb = tx.as<int32_t>(); }
        }
        const auto s_tab = sc.take<ImageGeom>((size_t)batch);
        const auto s_box = sc.take<int4>(n);
        const auto s_seg = sc.take<RleSeg>(n * RLE_SEGS);
        const auto s_run = sc.take<uint32_t>(n);
        sc.alloc();
        const ImageGeom* tab = sc[s_tab];
        int4* boxes = sc[s_box];
        RleSeg* segs = sc[s_seg];
        uint32_t* nruns = sc[s_run];
        if (batch > 0) HIP_CHECK(hipMemcpy(sc[s_tab], geom.data(), (size_t)batch * sizeof(ImageGeom), hipMemcpyHostToDevice));
        masks_rle_count_forward(st.s, d, m, tab, batch, rows, mask_size, model_h, model_w, threshold, ds, boxes, segs, nruns, ro, ar, bb);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + n, sizeof(need), hipMemcpyDeviceToHost, st.s));
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            if (n) HIP_CHECK(hipMemcpy(detections_src, ts.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(run_offsets, to.p, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost));
            if (areas && n) HIP_CHECK(hipMemcpy(areas, ta.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (bboxes_xywh && n) HIP_CHECK(hipMemcpy(bboxes_xywh, tx.p, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        MRCNN_REQUIRE(need <= (long long)capacity, MRCNN_ERR_SHAPE, "masks_rle_source: the batch encodes to %lld runs, counts holds %lld: call again with capacity >= %lld",
                      need, (long long)capacity, need);
        if (n == 0) return;
        uint32_t* c = counts;
        if (!dev) { tc.alloc((size_t)need * sizeof(uint32_t)); c = tc.as<uint32_t>(); }
        masks_rle_write_forward(st.s, m, tab, batch, rows, mask_size, threshold, boxes, segs, ro, c);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) HIP_CHECK(hipMemcpy(counts, tc.p, (size_t)need * sizeof(uint32_t), hipMemcpyDeviceToHost));    // only the used part crosses PCIe
    });
}

// ================================================================================================
// drawing (DetectionRenderer.swift:13-88): the instance-id map and the rendered overlay
// ================================================================================================
extern "C" int mrcnn_instance_map_source(const float* detections, const float* masks, int batch, int rows, int mask_size,
                                         const int32_t* heights, const int32_t* widths, int model_h, int model_w, float threshold,
                                         float min_score, int memspace, float* detections_src, int16_t* map, const int64_t* map_offsets,
                                         uint32_t* visible_areas)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(detections && masks && heights && widths && detections_src && map && map_offsets, MRCNN_ERR_INVALID, "null instance_map_source argument");
        MRCNN_REQUIRE(batch >= 0 && rows >= 0 && mask_size >= 2 && model_h > 0 && model_w > 0, MRCNN_ERR_INVALID, "bad instance_map_source argument");
        MRCNN_REQUIRE(rows <= 32767, MRCNN_ERR_SHAPE, "instance_map_source: %d rows do not fit the int16 map (at most 32767)", rows);
        MRCNN_REQUIRE((long)batch * rows < (1L << 31), MRCNN_ERR_SHAPE, "instance_map_source: %d x %d rows are too many", batch, rows);
        MRCNN_REQUIRE(reinterpret_cast<uintptr_t>(map) % 2 == 0, MRCNN_ERR_INVALID, "instance_map_source: map is not aligned for int16");
        if (batch == 0) return;
        int64_t extent = 0;
        long max_pixels = 0;
        const std::vector<ImageGeom> geom = image_geometry("instance_map_source", heights, widths, batch, model_h, model_w, map_offsets, 2, &extent, &max_pixels);
        const bool dev = memspace == MRCNN_DEVICE;
        Stream st;
        DevBuf td, tm, ts, tv;
        const size_t n = (size_t)batch * rows;
        const float* d = stage_rows(detections, memspace, (long)n, 6, 6, td);
        const float* m = stage_rows(masks, memspace, (long)n, (long)mask_size * mask_size, (long)mask_size * mask_size, tm);
        float* ds = detections_src;
        uint32_t* va = visible_areas;
        if (!dev) {
            ts.alloc((n ? n : 1) * 6 * sizeof(float)); ds = ts.as<float>();
            if (visible_areas) { tv.alloc((n ? n : 1) * sizeof(uint32_t)); va = tv.as<uint32_t>(); }
        }
        Carver sc;                                              // one scratch allocation: the geometry table | the pixel boxes
        const auto tab = sc.take<ImageGeom>((size_t)batch);
        const auto box = sc.take<int4>(n);
        sc.alloc();
        RaggedOut o(st.s, map, dev, extent);
        HIP_CHECK(hipMemcpy(sc[tab], geom.data(), (size_t)batch * sizeof(ImageGeom), hipMemcpyHostToDevice));
        instance_map_forward(st.s, d, m, sc[tab], batch, rows, mask_size, model_h, model_w, max_pixels, threshold, min_score, ds, sc[box],
                             reinterpret_cast<int16_t*>(o.p), va);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            if (n) HIP_CHECK(hipMemcpy(detections_src, ts.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost));
            if (visible_areas && n) HIP_CHECK(hipMemcpy(visible_areas, tv.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        o.deliver(map, map_offsets, heights, widths, batch, 2);
    });
}

extern "C" int mrcnn_render_detections_source(const mrcnn_image* images, const float* detections, const float* masks, int batch, int rows,
                                              int mask_size, int model_h, int model_w, float threshold, float min_score, int alpha, int stroke,
                                              int memspace, float* detections_src, uint8_t* out_rgb, const int64_t* out_offsets)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(images && detections && masks && out_rgb && out_offsets, MRCNN_ERR_INVALID, "null render_detections_source argument");
        MRCNN_REQUIRE(batch >= 0 && rows >= 0 && mask_size >= 2 && model_h > 0 && model_w > 0, MRCNN_ERR_INVALID, "bad render_detections_source argument");
        MRCNN_REQUIRE(rows <= 32767, MRCNN_ERR_SHAPE, "render_detections_source: %d rows are too many (at most 32767)", rows);
        MRCNN_REQUIRE((long)batch * rows < (1L << 31), MRCNN_ERR_SHAPE, "render_detections_source: %d x %d rows are too many", batch, rows);
        MRCNN_REQUIRE(alpha >= 0 && alpha <= 256, MRCNN_ERR_SHAPE, "render_detections_source: alpha %d outside 0..256", alpha);
        MRCNN_REQUIRE(stroke >= 0 && stroke <= 65534, MRCNN_ERR_SHAPE, "render_detections_source: stroke %d outside 0..65534", stroke);
        if (batch == 0) return;
        std::vector<int32_t> hs, ws;
        image_sizes(images, batch, "render_detections_source", hs, ws);
        int64_t extent = 0;
        long max_pixels = 0;
        const std::vector<ImageGeom> geom = image_geometry("render_detections_source", hs.data(), ws.data(), batch, model_h, model_w, out_offsets, 3, &extent, &max_pixels);
        const bool dev = memspace == MRCNN_DEVICE;
        Stream st;
        DevBuf td, tm, ts, ti;
        const size_t n = (size_t)batch * rows;
        const float* d = stage_rows(detections, memspace, (long)n, 6, 6, td);
        const float* m = stage_rows(masks, memspace, (long)n, (long)mask_size * mask_size, (long)mask_size * mask_size, tm);
        float* ds = detections_src;
        if (!dev || !detections_src) { ts.alloc((n ? n : 1) * 6 * sizeof(float)); ds = ts.as<float>(); }
        Carver sc;                                              // one scratch allocation: the geometry table | the source pointers | the pixel boxes
        const auto tab = sc.take<ImageGeom>((size_t)batch);
        const auto src = sc.take<const uint8_t*>((size_t)batch);
        const auto box = sc.take<int4>(n);
        sc.alloc();
        RaggedOut o(st.s, out_rgb, dev, extent);
        HIP_CHECK(hipMemcpy(sc[tab], geom.data(), (size_t)batch * sizeof(ImageGeom), hipMemcpyHostToDevice));
        upload_sources(images, batch, dev, ti, sc[src]);
        render_detections_forward(st.s, d, m, sc[tab], sc[src], batch, rows, mask_size, model_h, model_w, max_pixels, threshold, min_score, alpha, stroke, ds,
                                  sc[box], o.p);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev && detections_src && n) HIP_CHECK(hipMemcpy(detections_src, ts.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost));
        o.deliver(out_rgb, out_offsets, hs.data(), ws.data(), batch, 3);
    });
}

// COCO's compressed RLE string (pycocotools maskApi.c: rleToString / rleFrString) — host arithmetic, no GPU.  Counts from the fourth
// on go out as their difference to the count two places before; a value is written in 5-bit groups, low group first, 0x20 = more
// follows (until the rest is only the sign extension of the group's bit 0x10), character = group + 48.
extern "C" int mrcnn_rle_to_string(const uint32_t* counts, int64_t n, char* out, int64_t capacity, int64_t* length)
{
    return guarded([&] {
        MRCNN_REQUIRE(length && n >= 0 && (counts || n == 0) && capacity >= 0 && (out || capacity == 0), MRCNN_ERR_INVALID, "bad rle_to_string argument");
        int64_t p = 0;
        for (int64_t i = 0; i < n; ++i) {
            long long x = (long long)counts[i];
            if (i > 2) x -= (long long)counts[i - 2];
            bool more = true;
            while (more) {
                int c = (int)(x & 0x1f);
                x >>= 5;
                more = (c & 0x10) ? x != -1 : x != 0;
                if (more) c |= 0x20;
                if (p < capacity) out[p] = (char)(c + 48);
                ++p;
            }
        }
        *length = p;
        MRCNN_REQUIRE(p <= capacity || !out, MRCNN_ERR_SHAPE, "rle_to_string: the string has %lld characters, out holds %lld", (long long)p, (long long)capacity);
    });
}

extern "C" int mrcnn_rle_from_string(const char* s, int64_t length, uint32_t* counts, int64_t capacity, int64_t* n)
{
    return guarded([&] {
        MRCNN_REQUIRE(n && length >= 0 && (s || length == 0) && capacity >= 0 && (counts || capacity == 0), MRCNN_ERR_INVALID, "bad rle_from_string argument");
        int64_t m = 0, p = 0;
        long long before[2] = {0, 0};                     // the two counts before the current one (kept here: counts may be too short)
        while (p < length) {
            long long x = 0;
            int k = 0;
            bool more = true;
            while (more) {
                MRCNN_REQUIRE(p < length, MRCNN_ERR_INVALID, "rle_from_string: the string ends inside a value");
                const int c = (int)(unsigned char)s[p] - 48;
                MRCNN_REQUIRE(c >= 0 && c < 64 && k < 8, MRCNN_ERR_INVALID, "rle_from_string: character %lld is not part of an RLE string", (long long)p);
                x |= (long long)(c & 0x1f) << (5 * k);
                more = (c & 0x20) != 0;
                ++p; ++k;
                if (!more && (c & 0x10)) x |= -1LL << (5 * k);
            }
            if (m > 2) x += before[0];
            MRCNN_REQUIRE(x >= 0 && x <= 0xffffffffLL, MRCNN_ERR_INVALID, "rle_from_string: count %lld decodes to %lld", (long long)m, x);
            if (m < capacity) counts[m] = (uint32_t)x;
            before[0] = before[1]; before[1] = x;
            ++m;
        }
        *n = m;
        MRCNN_REQUIRE(m <= capacity || !counts, MRCNN_ERR_SHAPE, "rle_from_string: the string holds %lld counts, counts holds %lld", (long long)m, (long long)capacity);
    });
}
