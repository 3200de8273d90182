// api_polygons.hip — the C ABI of include/maskrcnn_hip.h, run-length masks to polygon rings: the host definition (polygons_host.cpp
// behind it) and the device entry (kernels_polygons.hip); the rings simplified: simplify_host.cpp and kernels_simplify.hip; and the rings
// nested into outlines and their holes: nest_host.cpp and kernels_nest.hip.  Every argument error is answered before a device is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "nest_host.h"
#include "polygons_host.h"
#include "simplify_host.h"
#include "simplify_rule.h"

using namespace mrcnn;

extern "C" int mrcnn_rle_to_polygons_host(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                          const int32_t* widths, int64_t* rle_rings, int64_t* n_rings, int64_t* n_vertices, int64_t* ring_offsets,
                                          int64_t* ring_areas, int64_t ring_capacity, int32_t* xy, int64_t vertex_capacity)
{
    return guarded([&] {
        const char* who = "rle_to_polygons_host";
        std::string err;
        const rle_draw::Set a{counts, run_offsets, n_images, slots, heights, widths};
        answer(polygons::check_arguments(a, rle_rings, n_rings, n_vertices, ring_offsets, ring_capacity, xy, vertex_capacity, who, &err), err);
        polygons::Rings r;
        answer(polygons::trace_host(a, who, &r, &err), err);
        const int64_t rings = (int64_t)r.ring_areas.size(), vertices = (int64_t)(r.xy.size() / 2);
        memcpy(rle_rings, r.rle_rings.data(), r.rle_rings.size() * sizeof(int64_t));
        *n_rings = rings; *n_vertices = vertices;
        answer(polygons::check_capacity(rings, vertices, ring_capacity, vertex_capacity, who, &err), err);
        if (ring_offsets) memcpy(ring_offsets, r.ring_offsets.data(), r.ring_offsets.size() * sizeof(int64_t));
        if (ring_areas && rings) memcpy(ring_areas, r.ring_areas.data(), (size_t)rings * sizeof(int64_t));
        if (xy && vertices) memcpy(xy, r.xy.data(), r.xy.size() * sizeof(int32_t));
    });
}

extern "C" int mrcnn_rle_to_polygons(const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights,
                                     const int32_t* widths, int memspace, int64_t* rle_rings, int64_t* n_rings, int64_t* n_vertices,
                                     int64_t* ring_offsets, int64_t* ring_areas, int64_t ring_capacity, int32_t* xy, int64_t vertex_capacity)
{
    return guarded([&] {
        const char* who = "rle_to_polygons";
        std::string err;
        const rle_draw::Set a{counts, run_offsets, n_images, slots, heights, widths};
        answer(polygons::check_arguments(a, rle_rings, n_rings, n_vertices, ring_offsets, ring_capacity, xy, vertex_capacity, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "%s: unknown memspace %d", who, memspace);
        const size_t n = (size_t)n_images * slots;
        std::vector<PolygonImage> tab((size_t)n_images);
        long long units = 0;
        for (int b = 0; b < n_images; ++b) {
            tab[(size_t)b] = PolygonImage{units, heights[b], widths[b]};
            units += (long long)slots * (widths[b] + 1);
        }
        MRCNN_REQUIRE(units < (1LL << 31), MRCNN_ERR_SHAPE, "%s: %d x %d RLEs have %lld pixel columns: too many", who, n_images, slots, units);
        if (memspace == MRCNN_HOST) answer(rle_draw::check_sums(a, who, &err), err);      // runs in host memory: a bad RLE needs no device to be named
        require_gpu();
        const bool dev = memspace == MRCNN_DEVICE;
        const auto put = [&](void* callers, const void* from, size_t bytes) {      // a result to the caller's memory space
            if (bytes) HIP_CHECK(hipMemcpy(callers, from, bytes, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
        };
        const int64_t zero = 0;
        if (n == 0) {
            put(rle_rings, &zero, sizeof zero);
            *n_rings = 0; *n_vertices = 0;
            if (ring_offsets) put(ring_offsets, &zero, sizeof zero);
            return;
        }

        Stream st;
        hipStream_t s = st.s;
        StagedRle in(counts, run_offsets, (int64_t)n, dev, who);
        DevBuf t_rings, t_offsets, t_areas, t_xy;
        Carver sc, wc;
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        in.stage();
        // one scratch allocation: the image table | totals | areas | the units' counts and prefix | the RLEs' first corners | the summary
        const auto s_tab = sc.take<PolygonImage>(tab.size());
        const auto s_tot = sc.take<unsigned long long>(n);
        const auto s_ar = sc.take<uint32_t>(n);
        const auto s_cnt = sc.take<uint32_t>((size_t)units);
        const auto s_start = sc.take<unsigned long long>((size_t)units + 1);
        const auto s_c0 = sc.take<long long>(n + 1);
        const auto s_sum = sc.take<unsigned long long>(3);
        sc.alloc();
        HIP_CHECK(hipMemcpy(sc[s_tab], tab.data(), tab.size() * sizeof(PolygonImage), hipMemcpyHostToDevice));
        const PolygonSet set{in.pre_b, in.run_offsets, sc[s_tot], sc[s_tab], n_images, slots, units, sc[s_cnt], sc[s_start], sc[s_c0]};
        rle_prefix_forward(s, in.counts, in.run_offsets, (long)n, in.pre_b, nullptr, sc[s_tot], sc[s_ar]);
        polygons_count_forward(s, set, sc[s_sum]);
        unsigned long long sum[3] = {0, 0, 0};                   // the first of the two read-backs: is every RLE right, and how large is the work
        const Refusal r = read_refusal(s, sc[s_sum], sc[s_tot], sum, sizeof sum);
        if (r.any) answer(rle_draw::bad_sum(a, r.k, r.sum, who, &err), err);   // nothing has been traced and nothing is written
        const long long corners = (long long)sum[1], most = (long long)sum[2];
        MRCNN_REQUIRE(corners < (1LL << 31), MRCNN_ERR_SHAPE, "%s: the set has %lld corners: too many for one call", who, corners);

        long long* d_rings = reinterpret_cast<long long*>(rle_rings);
        if (!dev) { t_rings.alloc((n + 1) * 8); d_rings = t_rings.as<long long>(); }
        long long rings = 0;
        PolygonWork w{};
        if (corners == 0) HIP_CHECK(hipMemsetAsync(d_rings, 0, (n + 1) * 8, s));
        else {
            const size_t c = (size_t)corners;
            const bool big = most > POLYGON_LDS_CORNERS;
            const auto w_corner = wc.take<uint32_t>(c), w_succ = wc.take<uint32_t>(c), w_lead = wc.take<uint32_t>(c), w_dist = wc.take<uint32_t>(c);
            const auto w_head = wc.take<uint32_t>(c), w_len = wc.take<uint32_t>(c);
            const auto w_id = wc.take<unsigned long long>(c + 1), w_v0 = wc.take<unsigned long long>(c + 1);
            const auto w_sort = wc.take<unsigned long long>(big ? 2 * c : 0), w_ps = wc.take<unsigned long long>(big ? n + 1 : 0);
            const auto w_pz = wc.take<uint32_t>(big ? n : 0), w_na = wc.take<uint32_t>(big ? c : 0), w_nb = wc.take<uint32_t>(big ? c : 0);
            const auto w_ma = wc.take<unsigned long long>(big ? c : 0), w_mb = wc.take<unsigned long long>(big ? c : 0);
            wc.alloc();
            w = PolygonWork{wc[w_corner], wc[w_succ], wc[w_lead], wc[w_dist], wc[w_head], wc[w_len], wc[w_id], wc[w_v0],
                            wc[w_sort], wc[w_pz], wc[w_ps], wc[w_na], wc[w_nb], wc[w_ma], wc[w_mb]};
            polygons_trace_forward(s, set, w, corners, most, d_rings);
            unsigned long long r = 0;                            // the second read-back: with the corners, the two totals of the capacity check
            HIP_CHECK(hipMemcpyAsync(&r, w.ring_id + c, sizeof r, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            rings = (long long)r;
        }
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(rle_rings, d_rings, (n + 1) * 8, hipMemcpyDeviceToHost));
        *n_rings = rings; *n_vertices = corners;
        answer(polygons::check_capacity(rings, corners, ring_capacity, vertex_capacity, who, &err), err);
        if (corners == 0) {
            if (ring_offsets) put(ring_offsets, &zero, sizeof zero);
            return;
        }
        long long* d_offsets = reinterpret_cast<long long*>(ring_offsets);
        long long* d_areas = reinterpret_cast<long long*>(ring_areas);
        int32_t* d_xy = xy;
        if (!dev) {
            t_offsets.alloc((size_t)(rings + 1) * 8); d_offsets = t_offsets.as<long long>();
            if (ring_areas) { t_areas.alloc((size_t)rings * 8); d_areas = t_areas.as<long long>(); }
            t_xy.alloc((size_t)corners * 8); d_xy = t_xy.as<int32_t>();
        }
        polygons_write_forward(s, w, corners, rings, d_offsets, d_areas, d_xy);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(ring_offsets, d_offsets, (size_t)(rings + 1) * 8, hipMemcpyDeviceToHost));
            if (ring_areas) HIP_CHECK(hipMemcpy(ring_areas, d_areas, (size_t)rings * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(xy, d_xy, (size_t)corners * 8, hipMemcpyDeviceToHost));
        }
    });
}

extern "C" int mrcnn_polygons_simplify_host(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance, int64_t* out_ring_offsets,
                                            int64_t* out_areas2, int32_t* out_xy, int64_t* out_src_index, int64_t* n_vertices_out,
                                            int64_t vertex_capacity)
{
    return guarded([&] {
        const char* who = "polygons_simplify_host";
        std::string err;
        answer(simplify::check_arguments(ring_offsets, xy, n_rings, tolerance, out_ring_offsets, out_xy, n_vertices_out, vertex_capacity, who, &err), err);
        int64_t most = 0;
        answer(simplify::check_offsets(ring_offsets, n_rings, who, &err, &most), err);
        answer(simplify::check_coordinates(ring_offsets, xy, n_rings, who, &err), err);
        simplify::Rings r;
        simplify::simplify_host(ring_offsets, xy, n_rings, simp_tolerance(tolerance), &r);
        const int64_t vertices = (int64_t)(r.xy.size() / 2);
        memcpy(out_ring_offsets, r.ring_offsets.data(), r.ring_offsets.size() * sizeof(int64_t));
        *n_vertices_out = vertices;
        answer(simplify::check_capacity(vertices, vertex_capacity, who, &err), err);
        if (out_areas2 && n_rings) memcpy(out_areas2, r.areas2.data(), (size_t)n_rings * sizeof(int64_t));
        if (vertices) memcpy(out_xy, r.xy.data(), r.xy.size() * sizeof(int32_t));
        if (out_src_index && vertices) memcpy(out_src_index, r.src_index.data(), (size_t)vertices * sizeof(int64_t));
    });
}

extern "C" int mrcnn_polygons_simplify(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance, int memspace,
                                       int64_t* out_ring_offsets, int64_t* out_areas2, int32_t* out_xy, int64_t* out_src_index,
                                       int64_t* n_vertices_out, int64_t vertex_capacity)
{
    return guarded([&] {
        const char* who = "polygons_simplify";
        std::string err;
        answer(simplify::check_arguments(ring_offsets, xy, n_rings, tolerance, out_ring_offsets, out_xy, n_vertices_out, vertex_capacity, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "%s: unknown memspace %d", who, memspace);
        MRCNN_REQUIRE(n_rings < (1LL << 31), MRCNN_ERR_SHAPE, "%s: %lld rings: too many for one call", who, (long long)n_rings);
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t n = (size_t)n_rings;
        int64_t most = 0, v_in = 0;
        if (!dev) {                                              // rings in host memory: a bad one needs no device to be named
            answer(simplify::check_offsets(ring_offsets, n_rings, who, &err, &most), err);
            answer(simplify::check_coordinates(ring_offsets, xy, n_rings, who, &err), err);
            v_in = ring_offsets[n];
        }
        const uint64_t E = simp_tolerance(tolerance);
        require_gpu();
        const int64_t zero = 0;
        if (n == 0) {
            HIP_CHECK(hipMemcpy(out_ring_offsets, &zero, sizeof zero, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
            *n_vertices_out = 0;
            return;
        }
        Stream st;
        hipStream_t s = st.s;
        DevBuf t_off, t_xy, t_out_off, t_areas, t_out_xy, t_src;
        Carver sc, wc;
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        SimplifyRings in{reinterpret_cast<const long long*>(ring_offsets), xy, (long long)n_rings};
        if (!dev) {                                              // (all of xy up to the last ring's end: the offsets hold as they are)
            t_off.alloc((n + 1) * 8); t_xy.alloc((size_t)v_in * 8);
            HIP_CHECK(hipMemcpy(t_off.p, ring_offsets, (n + 1) * 8, hipMemcpyHostToDevice));
            if (v_in) HIP_CHECK(hipMemcpy(t_xy.p, xy, (size_t)v_in * 8, hipMemcpyHostToDevice));
            in.ring_offsets = t_off.as<long long>(); in.xy = t_xy.as<int32_t>();
        }
        const auto s_sum = sc.take<unsigned long long>(4);
        const auto s_cnt = sc.take<uint32_t>(n);
        sc.alloc();
        if (dev) {                                               // the one read-back before anything is written: are the rings legal, how large are they
            simplify_check_forward(s, in, sc[s_sum]);
            unsigned long long sum[4] = {0, 0, 0, 0};
            HIP_CHECK(hipMemcpyAsync(sum, sc[s_sum], sizeof sum, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (sum[0] != ~0ull) answer(simplify::bad_offsets((int64_t)sum[0], who, &err), err);
            if (sum[1] != ~0ull) answer(simplify::bad_coordinate((int64_t)sum[1], who, &err), err);
            most = (int64_t)sum[2]; v_in = (int64_t)sum[3];
        }
        const bool big = most > SIMPLIFY_LDS_VERTICES;
        const size_t v = (size_t)v_in;
        const auto w_keep = wc.take<uint8_t>(v);
        const auto w_chain = wc.take<unsigned long long>(big ? v : 0), w_sa = wc.take<unsigned long long>(big ? v : 0);
        const auto w_sb = wc.take<unsigned long long>(big ? v : 0);
        wc.alloc();
        const SimplifyWork w{wc[w_keep], sc[s_cnt], big ? wc[w_chain] : nullptr, big ? wc[w_sa] : nullptr, big ? wc[w_sb] : nullptr};
        long long* d_out_off = reinterpret_cast<long long*>(out_ring_offsets);
        if (!dev) { t_out_off.alloc((n + 1) * 8); d_out_off = t_out_off.as<long long>(); }
        simplify_count_forward(s, in, E, w, d_out_off);
        long long needed = 0;                                    // the second read-back: the size the capacity is checked against
        HIP_CHECK(hipMemcpyAsync(&needed, d_out_off + n, sizeof needed, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(out_ring_offsets, d_out_off, (n + 1) * 8, hipMemcpyDeviceToHost));
        *n_vertices_out = needed;
        answer(simplify::check_capacity(needed, vertex_capacity, who, &err), err);
        long long* d_areas = reinterpret_cast<long long*>(out_areas2);
        long long* d_src = reinterpret_cast<long long*>(out_src_index);
        int32_t* d_xy = out_xy;
        if (!dev) {
            if (out_areas2) { t_areas.alloc(n * 8); d_areas = t_areas.as<long long>(); }
            if (out_src_index) { t_src.alloc((size_t)needed * 8); d_src = t_src.as<long long>(); }
            t_out_xy.alloc((size_t)needed * 8); d_xy = t_out_xy.as<int32_t>();
        }
        simplify_write_forward(s, in, w, d_out_off, needed, d_areas, d_xy, d_src);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            if (out_areas2) HIP_CHECK(hipMemcpy(out_areas2, d_areas, n * 8, hipMemcpyDeviceToHost));
            if (needed) HIP_CHECK(hipMemcpy(out_xy, d_xy, (size_t)needed * 8, hipMemcpyDeviceToHost));
            if (out_src_index && needed) HIP_CHECK(hipMemcpy(out_src_index, d_src, (size_t)needed * 8, hipMemcpyDeviceToHost));
        }
    });
}

extern "C" int mrcnn_polygons_nest_host(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings,
                                        int64_t* parent, int32_t* depth, int64_t* rle_polys, int64_t* poly_rings, int64_t* ring_order, int64_t* n_polys)
{
    return guarded([&] {
        const char* who = "polygons_nest_host";
        std::string err;
        answer(nest::check_arguments(rle_rings, n_rles, ring_offsets, xy, n_rings, parent, depth, rle_polys, poly_rings, ring_order, n_polys, who, &err), err);
        int64_t most = 0;
        answer(nest::check_rle_rings(rle_rings, n_rles, n_rings, who, &err), err);
        answer(simplify::check_offsets(ring_offsets, n_rings, who, &err, &most), err);
        answer(simplify::check_coordinates(ring_offsets, xy, n_rings, who, &err), err);
        nest::Nest t;
        nest::nest_host(rle_rings, n_rles, ring_offsets, xy, n_rings, &t);
        const size_t n = (size_t)n_rings;
        if (n) {
            memcpy(parent, t.parent.data(), n * sizeof(int64_t));
            memcpy(depth, t.depth.data(), n * sizeof(int32_t));
            memcpy(ring_order, t.ring_order.data(), n * sizeof(int64_t));
        }
        memcpy(rle_polys, t.rle_polys.data(), t.rle_polys.size() * sizeof(int64_t));
        memcpy(poly_rings, t.poly_rings.data(), t.poly_rings.size() * sizeof(int64_t));
        *n_polys = (int64_t)t.poly_rings.size() - 1;
    });
}

extern "C" int mrcnn_polygons_nest(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, int memspace,
                                   int64_t* parent, int32_t* depth, int64_t* rle_polys, int64_t* poly_rings, int64_t* ring_order, int64_t* n_polys)
{
    return guarded([&] {
        const char* who = "polygons_nest";
        std::string err;
        answer(nest::check_arguments(rle_rings, n_rles, ring_offsets, xy, n_rings, parent, depth, rle_polys, poly_rings, ring_order, n_polys, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "%s: unknown memspace %d", who, memspace);
        MRCNN_REQUIRE(n_rings < (1LL << 31) && n_rles < (1LL << 31) - 1, MRCNN_ERR_SHAPE, "%s: %lld rings in %lld RLEs: too many for one call", who,
                      (long long)n_rings, (long long)n_rles);
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t n = (size_t)n_rings, k = (size_t)n_rles;
        int64_t most = 0, v_in = 0;
        if (!dev) {                                              // rings in host memory: a bad one needs no device to be named
            answer(nest::check_rle_rings(rle_rings, n_rles, n_rings, who, &err), err);
            answer(simplify::check_offsets(ring_offsets, n_rings, who, &err, &most), err);
            answer(simplify::check_coordinates(ring_offsets, xy, n_rings, who, &err), err);
            v_in = ring_offsets[n];
        }
        require_gpu();
        Stream st;
        hipStream_t s = st.s;
        DevBuf t_rle, t_off, t_xy;
        Carver sc, oc;
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        NestRings in{reinterpret_cast<const long long*>(rle_rings), (long long)n_rles, reinterpret_cast<const long long*>(ring_offsets), xy, (long long)n_rings};
        if (!dev) {                                              // (all of xy up to the last ring's end: the offsets hold as they are)
            t_rle.alloc((k + 1) * 8); t_off.alloc((n + 1) * 8); t_xy.alloc((size_t)v_in * 8);
            HIP_CHECK(hipMemcpy(t_rle.p, rle_rings, (k + 1) * 8, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(t_off.p, ring_offsets, (n + 1) * 8, hipMemcpyHostToDevice));
            if (v_in) HIP_CHECK(hipMemcpy(t_xy.p, xy, (size_t)v_in * 8, hipMemcpyHostToDevice));
            in.rle_rings = t_rle.as<long long>(); in.ring_offsets = t_off.as<long long>(); in.xy = t_xy.as<int32_t>();
        }
        // one scratch allocation: the summary | per ring its size, box, RLE, the three counts | the two prefix sums
        const auto s_sum = sc.take<unsigned long long>(3);
        const auto s_size = sc.take<unsigned long long>(n);
        const auto s_box = sc.take<int4>(n);
        const auto s_rle = sc.take<int32_t>(n);
        const auto s_shell = sc.take<uint32_t>(n), s_holes = sc.take<uint32_t>(n), s_rings = sc.take<uint32_t>(n);
        const auto s_polygon = sc.take<unsigned long long>(n + 1), s_start = sc.take<unsigned long long>(n + 1);
        sc.alloc();
        const NestWork w{sc[s_size], sc[s_box], sc[s_rle], sc[s_shell], sc[s_holes], sc[s_rings], sc[s_polygon], sc[s_start]};
        nest_measure_forward(s, in, w, sc[s_sum]);
        unsigned long long sum[3] = {0, 0, 0};                   // the one read-back before anything is written: are the rings legal
        HIP_CHECK(hipMemcpyAsync(sum, sc[s_sum], sizeof sum, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (sum[0] != ~0ull) answer(nest::bad_rle_rings((int64_t)sum[0], n_rings, who, &err), err);
        if (sum[1] != ~0ull) answer(simplify::bad_offsets((int64_t)sum[1], who, &err), err);
        if (sum[2] != ~0ull) answer(simplify::bad_coordinate((int64_t)sum[2], who, &err), err);
        if (n == 0) {                                            // no rings: no polygons in any RLE
            if (dev) HIP_CHECK(hipMemset(rle_polys, 0, (k + 1) * 8));
            else memset(rle_polys, 0, (k + 1) * 8);
            HIP_CHECK(hipMemcpy(poly_rings, rle_polys, 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost));
            *n_polys = 0;
            return;
        }
        long long *d_parent = reinterpret_cast<long long*>(parent), *d_polys = reinterpret_cast<long long*>(rle_polys);
        long long *d_rings = reinterpret_cast<long long*>(poly_rings), *d_order = reinterpret_cast<long long*>(ring_order);
        int32_t* d_depth = depth;
        const auto o_parent = oc.take<long long>(dev ? 0 : n), o_polys = oc.take<long long>(dev ? 0 : k + 1), o_rings = oc.take<long long>(dev ? 0 : n + 1);
        const auto o_order = oc.take<long long>(dev ? 0 : n);
        const auto o_depth = oc.take<int32_t>(dev ? 0 : n);
        if (!dev) {
            oc.alloc();
            d_parent = oc[o_parent]; d_polys = oc[o_polys]; d_rings = oc[o_rings]; d_order = oc[o_order]; d_depth = oc[o_depth];
        }
        nest_forward(s, in, w, d_parent, d_depth, d_polys, d_rings, d_order);
        unsigned long long polys = 0;                            // the second read-back: the number of polygons
        HIP_CHECK(hipMemcpyAsync(&polys, w.polygon + n, sizeof polys, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(parent, d_parent, n * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(depth, d_depth, n * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(rle_polys, d_polys, (k + 1) * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(poly_rings, d_rings, (size_t)(polys + 1) * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ring_order, d_order, n * 8, hipMemcpyDeviceToHost));
        }
        *n_polys = (int64_t)polys;
    });
}
