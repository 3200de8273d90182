// api_rle_shape.hip — the C ABI of include/maskrcnn_hip.h, measuring run-length masks: moments and perimeter (mrcnn_rle_measure), convex
// hull and oriented box (mrcnn_rle_convex_hull) of every RLE of a flat set — the host definitions (rle_shape_host.cpp behind them) and the
// device entries (kernels_rle_shape.hip).  Every argument error is answered before a device is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "rle_shape_host.h"
#include "shape_rule.h"

using namespace mrcnn;

namespace {

// What both device entries do first: the set staged on the device, its prefix table, and the one read-back before anything is written —
// the flag that refuses an RLE which does not sum to its plane.
struct ShapeCall {
    StagedRle in;
    Carver sc;
    ShapeSet S{};
    int max_w = 0;

    ShapeCall(const rle_shape::Set& a, bool dev, const char* who) : in(a.counts, a.run_offsets, a.n, dev, who) {}

    void stage(hipStream_t s, const rle_shape::Set& a, const char* who)
    {
        std::string err;
        const size_t N = (size_t)a.n;
        in.stage();
        std::vector<long long> vcol0(N + 1, 0);
        for (size_t k = 0; k < N; ++k) {
            vcol0[k + 1] = vcol0[k] + a.widths[k] + 1;
            max_w = std::max(max_w, (int)a.widths[k]);
        }
        // one scratch allocation: heights | widths | vertex columns | totals | areas | the flag
        const auto s_h = sc.take<int32_t>(N), s_w = sc.take<int32_t>(N);
        const auto s_v = sc.take<long long>(N + 1);
        const auto s_tot = sc.take<unsigned long long>(N);
        const auto s_ar = sc.take<uint32_t>(N);
        const auto s_bad = sc.take<unsigned long long>(1);
        sc.alloc();
        HIP_CHECK(hipMemcpy(sc[s_h], a.heights, N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(sc[s_w], a.widths, N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(sc[s_v], vcol0.data(), (N + 1) * 8, hipMemcpyHostToDevice));
        rle_prefix_forward(s, in.counts, in.run_offsets, (long)a.n, in.pre_b, nullptr, sc[s_tot], sc[s_ar]);
        S = ShapeSet{in.counts, in.pre_b, in.run_offsets, sc[s_h], sc[s_w], sc[s_tot], sc[s_v], (int)a.n, vcol0[N]};
        rle_shape_check_forward(s, S, sc[s_bad]);
        const Refusal r = read_refusal(s, sc[s_bad], sc[s_tot]);
        if (r.any) answer(rle_set::bad_sum(a, r.k, r.sum, who, &err), err);
    }
};

}  // namespace

extern "C" int mrcnn_rle_measure_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                      int64_t* measures)
{
    return guarded([&] {
        std::string err;
        answer(rle_shape::measure_host(rle_shape::Set{counts, run_offsets, n, heights, widths}, measures, &err), err);
    });
}

extern "C" int mrcnn_rle_measure(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                 int memspace, int64_t* measures)
{
    return guarded([&] {
        const char* who = "rle_measure";
        std::string err;
        const rle_shape::Set a{counts, run_offsets, n, heights, widths};
        answer(rle_set::check_flat(a, who, &err), err);
        MRCNN_REQUIRE(measures || n == 0, MRCNN_ERR_INVALID, "%s: null measures", who);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "%s: unknown memspace %d", who, memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);     // the offsets can be judged here: before a device is looked for
        require_gpu();
        if (n == 0) return;
        Stream st;
        ShapeCall call(a, dev, who);
        DevBuf tm;
        Drain drain{st.s};
        call.stage(st.s, a, who);
        const size_t bytes = (size_t)n * SHAPE_MEASURE_WORDS * sizeof(long long);
        long long* m = reinterpret_cast<long long*>(measures);
        if (!dev) { tm.alloc(bytes); m = tm.as<long long>(); }
        rle_shape_measure_forward(st.s, call.S, m);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) HIP_CHECK(hipMemcpy(measures, tm.p, bytes, hipMemcpyDeviceToHost));
    });
}

extern "C" int mrcnn_rle_convex_hull_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                          const int32_t* widths, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy,
                                          int64_t* n_vertices, int64_t vertex_capacity)
{
    return guarded([&] {
        std::string err;
        answer(rle_shape::convex_hull_host(rle_shape::Set{counts, run_offsets, n, heights, widths}, hull_offsets, hull_areas2, obb, xy, n_vertices,
                                           vertex_capacity, &err), err);
    });
}

extern "C" int mrcnn_rle_convex_hull(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                     int memspace, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy, int64_t* n_vertices,
                                     int64_t vertex_capacity)
{
    return guarded([&] {
        const char* who = "rle_convex_hull";
        std::string err;
        const rle_shape::Set a{counts, run_offsets, n, heights, widths};
        answer(rle_set::check_flat(a, who, &err), err);
        answer(rle_shape::check_hull_arguments(hull_offsets, xy, n_vertices, vertex_capacity, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "%s: unknown memspace %d", who, memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);
        require_gpu();
        const size_t N = (size_t)n;
        if (n == 0) {
            const int64_t zero = 0;
            HIP_CHECK(hipMemcpy(hull_offsets, &zero, sizeof zero, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
            *n_vertices = 0;
            return;
        }
        Stream st;
        hipStream_t s = st.s;
        ShapeCall call(a, dev, who);
        DevBuf t_off, t_areas, t_obb, t_xy;
        Carver wc;
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        call.stage(s, a, who);
        const ShapeSet& S = call.S;
        const bool big = call.max_w + 1 > HULL_LDS_COLUMNS;
        const size_t v = (size_t)S.vcols;
        const auto w_ext = wc.take<int2>(v);
        const auto w_keep = wc.take<uint8_t>(2 * v);
        const auto w_cnt = wc.take<uint32_t>(N);
        const auto w_chain = wc.take<uint32_t>(big ? 2 * v : 0);
        const auto w_slot = wc.take<unsigned long long>(big ? 2 * v : 0);
        wc.alloc();
        const HullWork W{wc[w_ext], wc[w_keep], wc[w_cnt], big ? wc[w_chain] : nullptr, big ? wc[w_slot] : nullptr};
        long long* d_off = reinterpret_cast<long long*>(hull_offsets);
        if (!dev) { t_off.alloc((N + 1) * 8); d_off = t_off.as<long long>(); }
        rle_hull_count_forward(s, S, W, call.max_w, d_off);
        long long need = 0;                                      // the second read-back: the size the capacity is checked against
        HIP_CHECK(hipMemcpyAsync(&need, d_off + N, sizeof need, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(hull_offsets, d_off, (N + 1) * 8, hipMemcpyDeviceToHost));
        *n_vertices = need;
        // The rings are written to a buffer of this call's own: the areas and the boxes are made from them whatever the capacity, and the
        // caller's xy gets them only when all fit.
        long long* d_areas = reinterpret_cast<long long*>(hull_areas2);
        long long* d_obb = reinterpret_cast<long long*>(obb);
        if (!dev) {
            if (hull_areas2) { t_areas.alloc(N * 8); d_areas = t_areas.as<long long>(); }
            if (obb) { t_obb.alloc(N * SHAPE_OBB_WORDS * 8); d_obb = t_obb.as<long long>(); }
        }
        t_xy.alloc((size_t)(need ? need : 1) * 8);
        rle_hull_write_forward(s, S, W, d_off, need, t_xy.as<int32_t>(), d_areas, d_obb);
        const bool fits = need <= (long long)vertex_capacity;
        if (fits && need) HIP_CHECK(hipMemcpyAsync(xy, t_xy.p, (size_t)need * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            if (hull_areas2) HIP_CHECK(hipMemcpy(hull_areas2, d_areas, N * 8, hipMemcpyDeviceToHost));
            if (obb) HIP_CHECK(hipMemcpy(obb, d_obb, N * SHAPE_OBB_WORDS * 8, hipMemcpyDeviceToHost));
        }
        if (!fits) answer(rle_shape::bad_capacity(need, (long long)vertex_capacity, who, &err), err);
    });
}
