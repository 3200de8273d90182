// api_tiles.hip — the C ABI of include/maskrcnn_hip.h, tiled prediction: the planner, the host merge and the host union (tiles_host.cpp
// behind them), the predict over windows (Model::predict_tiles), and the device merge and the device union (kernels_tiles.hip), which
// share one staging (TilesRun).  Every argument error is answered before a device is looked for.
#include "api_util.h"
#include "kernels_tiles.h"
#include "tiles_host.h"

using namespace mrcnn;

extern "C" int mrcnn_tile_plan(int height, int width, int tile_h, int tile_w, int overlap_y, int overlap_x, int image, mrcnn_tile* out,
                               int capacity, int* count)
{
    return guarded([&] {
        std::string err;
        answer(tiles::plan(height, width, tile_h, tile_w, overlap_y, overlap_x, image, out, capacity, count, &err), err);
    });
}

extern "C" int mrcnn_maskrcnn_predict_tiles(mrcnn_model* model, const mrcnn_image* images, int n_images, const mrcnn_tile* tiles, int n_tiles,
                                            int memspace, float* detections, float* masks)
{
    return guarded([&] {
        MRCNN_REQUIRE(model && images && tiles && detections && masks, MRCNN_ERR_INVALID, "predict_tiles: null argument");
        MRCNN_REQUIRE(n_tiles >= 1, MRCNN_ERR_SHAPE, "predict_tiles: n_tiles %d < 1", n_tiles);
        MRCNN_REQUIRE(n_images >= 1, MRCNN_ERR_SHAPE, "predict_tiles: n_images %d < 1", n_images);
        std::vector<int32_t> hs, ws;
        image_sizes(images, n_images, "predict_tiles", hs, ws);
        std::string err;
        answer(tiles::check_tiles(tiles, n_tiles, hs.data(), ws.data(), n_images, "predict_tiles", &err), err);
        model->m.predict_tiles(images, n_images, tiles, n_tiles, memspace, detections, masks);
    });
}

static tiles::MergeArgs merge_args(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                   const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold, int metric,
                                   double match_threshold, int max_out, float* detections_src, int32_t* source, int32_t* n_kept, uint32_t* counts,
                                   int64_t capacity, int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh, int32_t* n_parts = nullptr,
                                   int32_t* group = nullptr)
{
    return tiles::MergeArgs{detections, masks, tiles, n_tiles, rows, mask_size, heights, widths, n_images, model_h, model_w, threshold, metric,
                            match_threshold, max_out, detections_src, source, n_kept, counts, capacity, run_offsets, areas, bboxes_xywh, n_parts, group};
}

extern "C" int mrcnn_merge_tiles_host(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                      const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold,
                                      int metric, double match_threshold, int max_out, float* detections_src, int32_t* source, int32_t* n_kept,
                                      uint32_t* counts, int64_t capacity, int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(tiles::merge_host(merge_args(detections, masks, tiles, n_tiles, rows, mask_size, heights, widths, n_images, model_h, model_w,
                                                    threshold, metric, match_threshold, max_out, detections_src, source, n_kept, counts, capacity,
                                                    run_offsets, areas, bboxes_xywh), &err), err);
    });
}

extern "C" int mrcnn_unite_tiles_host(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                      const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold,
                                      int metric, double link_threshold, int max_out, float* detections_src, int32_t* source, int32_t* n_kept,
                                      int32_t* n_parts, int32_t* group, uint32_t* counts, int64_t capacity, int64_t* run_offsets, uint32_t* areas,
                                      int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(tiles::unite_host(merge_args(detections, masks, tiles, n_tiles, rows, mask_size, heights, widths, n_images, model_h, model_w,
                                                    threshold, metric, link_threshold, max_out, detections_src, source, n_kept, counts, capacity,
                                                    run_offsets, areas, bboxes_xywh, n_parts, group), &err), err);
    });
}

namespace {

// One merge / unite call on the device.  The constructor stages what both entries share: the tables, the candidates' boxes in the full
// frame, their planes as runs and the per-image order (steps 1 to 3 of kernels_tiles.hip).  The entry then runs its own selection,
// deliver() hands out the fixed-size results and checks the capacity, and the entry's write step fills out_counts before done().
struct TilesRun {
    const tiles::MergeArgs& a;
    const char* who;
    const bool dev, unite;
    const size_t n, slots;
    Stream st_;
    DevBuf td, tm, tc, toc;
    Carver tt, tw;                                           // one allocation for the tables, one for the scratch
    Drain drain;                                             // (declared behind the buffers: the stream drains before they are freed)
    TilesMerge m{};
    hipStream_t s;

    TilesRun(const tiles::MergeArgs& args, int memspace, const char* name, bool uniting)
        : a(args), who(name), dev(memspace == MRCNN_DEVICE), unite(uniting), n((size_t)args.n_tiles * args.rows),
          slots((size_t)args.n_images * args.max_out), drain{st_.s}, s(st_.s)
    {
        const int n_tiles = a.n_tiles, n_images = a.n_images, rows = a.rows;
        // the host tables: per tile its own letterbox geometry (the box map), its image's size (the RLE kernels) and its place; per image its tiles
        std::vector<ImageGeom> tab((size_t)2 * n_tiles);
        std::vector<TileGeom> tg((size_t)n_tiles);
        std::vector<int> toff((size_t)n_images + 1, 0), tlist((size_t)n_tiles);
        std::vector<int2> imgsz((size_t)n_images);
        for (int b = 0; b < n_images; ++b) imgsz[(size_t)b] = make_int2(a.heights[b], a.widths[b]);
        for (int t = 0; t < n_tiles; ++t) {
            const mrcnn_tile& w = a.tiles[t];
            ImageGeom& g = tab[(size_t)t];
            g = ImageGeom{};
            g.h = w.height; g.w = w.width; g.pitch = w.width;
            MRCNN_REQUIRE(mrcnn_letterbox_geometry(g.h, g.w, a.model_h, a.model_w, &g.nh, &g.nw, &g.py, &g.px) == MRCNN_OK, MRCNN_ERR_INVALID,
                          "%s: tile %d: bad letterbox geometry", who, t);
            ImageGeom& f = tab[(size_t)n_tiles + t];
            f = ImageGeom{};
            f.h = a.heights[w.image]; f.w = a.widths[w.image]; f.pitch = f.w;
            tg[(size_t)t] = TileGeom{w.image, w.y0, w.x0, f.h, f.w, w.height, w.width};
            ++toff[(size_t)w.image + 1];
        }
        int most = 0;
        for (int b = 0; b < n_images; ++b) { most = std::max(most, toff[(size_t)b + 1] * rows); toff[(size_t)b + 1] += toff[(size_t)b]; }
        {
            std::vector<int> fill(toff.begin(), toff.end() - 1);
            for (int t = 0; t < n_tiles; ++t) tlist[(size_t)fill[(size_t)a.tiles[t].image]++] = t;         // ascending t within an image
        }
        m.n_tiles = n_tiles; m.rows = rows; m.S = a.mask_size; m.n_images = n_images; m.max_out = a.max_out; m.W = (most + 63) / 64;
        m.thr = a.threshold; m.metric = a.metric; m.match_thr = a.match_threshold;
        m.det = stage_rows(a.detections, memspace, (long)n, 6, 6, td);
        m.masks = stage_rows(a.masks, memspace, (long)n, (long)a.mask_size * a.mask_size, (long)a.mask_size * a.mask_size, tm);
        auto table = [&](auto slot, const auto& v) {
            HIP_CHECK(hipMemcpyAsync(tt[slot], v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, s));
            return tt[slot];
        };
        const auto s_tab = tt.take<ImageGeom>(tab.size());
        const auto s_tg = tt.take<TileGeom>(tg.size());
        const auto s_toff = tt.take<int>(toff.size()), s_tl = tt.take<int>(tlist.size());
        const auto s_sz = tt.take<int2>(imgsz.size());
        tt.alloc();
        const ImageGeom* tab_tile = table(s_tab, tab);
        m.tab_full = tab_tile + n_tiles;
        m.tiles = table(s_tg, tg);
        m.toff = table(s_toff, toff);
        m.tlist = table(s_tl, tlist);
        m.imgsz = table(s_sz, imgsz);
        HIP_CHECK(hipStreamSynchronize(s));                      // (the vectors above are pageable: the copies have read them now)
        // the scratch; the outputs are the caller's device arrays, or a staging copy of each; u: the union's member lists, hulls and
        // segments, and its two outputs
        const size_t u = unite ? 1 : 0;
        const auto w_box = tw.take<int4>(n);
        const auto w_rows = tw.take<float>(n * 6), w_tile = tw.take<float>(n * 6), w_ds = tw.take<float>(slots * 6);
        const auto w_seg = tw.take<RleSeg>(n * RLE_SEGS), w_oseg = tw.take<RleSeg>(u * slots * RLE_SEGS);
        const auto w_nr = tw.take<uint32_t>(n), w_ar = tw.take<uint32_t>(n), w_onr = tw.take<uint32_t>(slots), w_oar = tw.take<uint32_t>(slots);
        const auto w_ro = tw.take<long long>(n + 1), w_oro = tw.take<long long>(slots + 1);
        const auto w_bb = tw.take<int32_t>(n * 4), w_ord = tw.take<int32_t>(n), w_pos = tw.take<int32_t>(n), w_ne = tw.take<int32_t>((size_t)n_images),
                   w_src = tw.take<int32_t>(slots), w_nk = tw.take<int32_t>((size_t)n_images), w_obb = tw.take<int32_t>(slots * 4),
                   w_mem = tw.take<int32_t>(u * n), w_np = tw.take<int32_t>(u * slots), w_grp = tw.take<int32_t>(u * n);
        const auto w_sup = tw.take<unsigned long long>(n * (size_t)m.W);
        const auto w_span = tw.take<int2>(u * slots);
        const auto w_hull = tw.take<int4>(u * slots);
        tw.alloc();
        m.boxes = tw[w_box]; m.rows_src = tw[w_rows];
        m.segs = tw[w_seg]; m.nruns = tw[w_nr]; m.ro = tw[w_ro];
        m.areas = tw[w_ar]; m.bboxes = tw[w_bb];
        m.order = tw[w_ord]; m.pos = tw[w_pos]; m.nelig = tw[w_ne];
        m.supp = tw[w_sup]; m.out_nruns = tw[w_onr];
        m.det_src = dev ? a.detections_src : tw[w_ds];
        m.source = dev ? a.source : tw[w_src];
        m.n_kept = dev ? a.n_kept : tw[w_nk];
        m.out_ro = dev ? reinterpret_cast<long long*>(a.run_offsets) : tw[w_oro];
        m.out_areas = dev && a.areas ? a.areas : tw[w_oar];
        m.out_bboxes = dev && a.bboxes_xywh ? a.bboxes_xywh : tw[w_obb];
        if (unite) {
            m.members = tw[w_mem]; m.mspan = tw[w_span];
            m.hull = tw[w_hull]; m.out_segs = tw[w_oseg];
            m.n_parts = dev && a.n_parts ? a.n_parts : tw[w_np];
            m.group = dev && a.group ? a.group : tw[w_grp];
        }
        // 1. the boxes, 2. the candidates' runs counted
        unletterbox_boxes_forward(s, m.det, tab_tile, n_tiles, rows, a.model_h, a.model_w, tw[w_tile], m.boxes);
        tiles_rle_count_forward(s, m);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, m.ro + n, sizeof need, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        tc.alloc((size_t)need * sizeof(uint32_t));
        m.counts = tc.as<uint32_t>();
        // 3. the runs and the per-image order
        tiles_order_forward(s, m);
    }

    // the selection has run: the fixed-size results to the caller, the capacity checked, out_counts ready for the write step
    void deliver()
    {
        long long out_need = 0;
        HIP_CHECK(hipMemcpyAsync(&out_need, m.out_ro + slots, sizeof out_need, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(a.detections_src, m.det_src, slots * 6 * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(a.source, m.source, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(a.n_kept, m.n_kept, (size_t)a.n_images * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(a.run_offsets, m.out_ro, (slots + 1) * sizeof(long long), hipMemcpyDeviceToHost));
            if (a.areas) HIP_CHECK(hipMemcpy(a.areas, m.out_areas, slots * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (a.bboxes_xywh) HIP_CHECK(hipMemcpy(a.bboxes_xywh, m.out_bboxes, slots * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (unite && a.n_parts) HIP_CHECK(hipMemcpy(a.n_parts, m.n_parts, slots * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (unite && a.group) HIP_CHECK(hipMemcpy(a.group, m.group, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        MRCNN_REQUIRE(out_need <= (long long)a.capacity, MRCNN_ERR_SHAPE, "%s: the kept masks encode to %lld runs, counts holds %lld: call again with capacity >= %lld",
                      who, out_need, (long long)a.capacity, out_need);
        m.out_counts = a.counts;
        if (!dev) { toc.alloc((size_t)out_need * sizeof(uint32_t)); m.out_counts = toc.as<uint32_t>(); }
        used = out_need;
    }

    // the write step is queued: the runs to the caller
    void done()
    {
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(a.counts, toc.p, (size_t)used * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }

    long long used = 0;
};

}  // namespace

extern "C" int mrcnn_merge_tiles(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                 const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold, int metric,
                                 double match_threshold, int max_out, int memspace, float* detections_src, int32_t* source, int32_t* n_kept,
                                 uint32_t* counts, int64_t capacity, int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        const tiles::MergeArgs a = merge_args(detections, masks, tiles, n_tiles, rows, mask_size, heights, widths, n_images, model_h, model_w, threshold,
                                              metric, match_threshold, max_out, detections_src, source, n_kept, counts, capacity, run_offsets, areas,
                                              bboxes_xywh);
        answer(tiles::check_merge(a, "merge_tiles", &err), err);
        require_gpu();
        TilesRun r(a, memspace, "merge_tiles", false);
        tiles_select_forward(r.s, r.m);                          // 4., 5. suppression bits, greedy scan, the size of the output
        r.deliver();
        tiles_gather_forward(r.s, r.m);
        r.done();
    });
}

extern "C" int mrcnn_unite_tiles(const float* detections, const float* masks, const mrcnn_tile* tiles, int n_tiles, int rows, int mask_size,
                                 const int32_t* heights, const int32_t* widths, int n_images, int model_h, int model_w, float threshold, int metric,
                                 double link_threshold, int max_out, int memspace, float* detections_src, int32_t* source, int32_t* n_kept,
                                 int32_t* n_parts, int32_t* group, uint32_t* counts, int64_t capacity, int64_t* run_offsets, uint32_t* areas,
                                 int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        const tiles::MergeArgs a = merge_args(detections, masks, tiles, n_tiles, rows, mask_size, heights, widths, n_images, model_h, model_w, threshold,
                                              metric, link_threshold, max_out, detections_src, source, n_kept, counts, capacity, run_offsets, areas,
                                              bboxes_xywh, n_parts, group);
        answer(tiles::check_merge(a, "unite_tiles", &err, "link_threshold"), err);
        require_gpu();
        TilesRun r(a, memspace, "unite_tiles", true);
        tiles_unite_forward(r.s, r.m);                           // link bits, components, the union planes counted
        r.deliver();
        tiles_unite_write_forward(r.s, r.m);
        r.done();
    });
}
