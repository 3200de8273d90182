// api_polygons.hip — the C ABI of include/maskrcnn_hip.h, run-length masks to polygon rings: the host definition (polygons_host.cpp
// behind it) and the device entry (kernels_polygons.hip).  Every argument error is answered before a device is looked for.
#include <string.h>

#include "api_util.h"
#include "polygons_host.h"

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

        // the set on the device and its run offsets here, as the drawing entries stage them
        std::vector<long long> h_off(n + 1, 0);
        if (dev) HIP_CHECK(hipMemcpy(h_off.data(), run_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
        else memcpy(h_off.data(), run_offsets, (n + 1) * 8);
        answer(rle_draw::check_run_offsets(reinterpret_cast<const int64_t*>(h_off.data()), (int64_t)n, who, &err), err);
        for (size_t k = 0; k < n; ++k)
            MRCNN_REQUIRE(h_off[k + 1] - h_off[k] < (1LL << 31), MRCNN_ERR_SHAPE, "%s: RLE %lld has %lld runs: too many", who, (long long)k, h_off[k + 1] - h_off[k]);
        const size_t runs = (size_t)h_off[n];
        MRCNN_REQUIRE(counts || runs == 0, MRCNN_ERR_INVALID, "%s: null counts", who);
        Stream st;
        hipStream_t s = st.s;
        DevBuf tc, to, tp, t_rings, t_offsets, t_areas, t_xy;
        Carver sc, wc;
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        const uint32_t* d_counts = counts;
        const long long* d_off = reinterpret_cast<const long long*>(run_offsets);
        if (!dev) {
            tc.alloc(runs * 4); to.alloc((n + 1) * 8);
            if (runs) HIP_CHECK(hipMemcpy(tc.p, counts, runs * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(to.p, h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
            d_counts = tc.as<uint32_t>(); d_off = to.as<long long>();
        }
        tp.alloc(runs * 4);
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
        const PolygonSet set{tp.as<uint32_t>(), d_off, sc[s_tot], sc[s_tab], n_images, slots, units, sc[s_cnt], sc[s_start], sc[s_c0]};
        rle_prefix_forward(s, d_counts, d_off, (long)n, tp.as<uint32_t>(), nullptr, sc[s_tot], sc[s_ar]);
        polygons_count_forward(s, set, sc[s_sum]);
        unsigned long long sum[3] = {0, 0, 0};                   // the first of the two read-backs: is every RLE right, and how large is the work
        HIP_CHECK(hipMemcpyAsync(sum, sc[s_sum], sizeof sum, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (sum[0] != ~0ull) {                                   // nothing has been traced and nothing is written
            const unsigned long long k = sum[0];
            unsigned long long total = 0;
            HIP_CHECK(hipMemcpy(&total, sc[s_tot] + k, sizeof total, hipMemcpyDeviceToHost));
            const int b = (int)(k / (unsigned long long)slots);
            fail(MRCNN_ERR_SHAPE, "%s: RLE %llu (image %d, slot %d) sums to %llu pixels, its %dx%d plane has %llu", who, k, b,
                 (int)(k % (unsigned long long)slots), total, heights[b], widths[b], (unsigned long long)heights[b] * (unsigned long long)widths[b]);
        }
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
