// api_rle_morph.hip — the C ABI of include/maskrcnn_hip.h, changing run-length masks: erosion, dilation and the boundary band of an RLE
// set — the host definition (rle_morph_host.cpp behind it), the device entry (kernels_rle_morph.hip) and the radius Boundary IoU takes
// from an image's diagonal.  Every argument error is answered before a device is looked for.
#include <math.h>
#include <string.h>

#include "api_util.h"
#include "rle_draw_host.h"
#include "rle_morph_host.h"

using namespace mrcnn;

extern "C" int mrcnn_boundary_radius(int h, int w, double ratio, int32_t* radius)
{
    return guarded([&] {
        MRCNN_REQUIRE(radius, MRCNN_ERR_INVALID, "boundary_radius: null radius");
        MRCNN_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, MRCNN_ERR_SHAPE, "boundary_radius: the image is %dx%d: height and width must lie in 1..32767", h, w);
        MRCNN_REQUIRE(isfinite(ratio) && ratio > 0.0, MRCNN_ERR_SHAPE, "boundary_radius: ratio %g is not finite and > 0", ratio);
        *radius = morph_boundary_radius(h, w, ratio);
    });
}

extern "C" int mrcnn_rle_morph_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                    const int32_t* radii, int op, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas,
                                    int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(rle_morph::morph_host(rle_morph::Set{counts, run_offsets, n, heights, widths, radii, op}, out_counts, capacity, out_run_offsets, areas,
                                     bboxes_xywh, &err), err);
    });
}

extern "C" int mrcnn_rle_morph(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                               const int32_t* radii, int op, int memspace, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets,
                               uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        const char* who = "rle_morph";
        std::string err;
        const rle_morph::Set a{counts, run_offsets, n, heights, widths, radii, op};
        answer(rle_morph::check_arguments(a, out_counts, capacity, out_run_offsets, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_morph: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) {                                              // the offsets can be judged here: before a device is looked for
            answer(rle_draw::check_run_offsets(run_offsets, n, who, &err), err);
            MRCNN_REQUIRE(counts || run_offsets[n] == run_offsets[0], MRCNN_ERR_INVALID, "rle_morph: null counts");
        }
        require_gpu();
        Stream st;
        DevBuf tc, to, tp, tro, tar, tbb, tcnt, bits;
        Carver sc;
        Drain drain{st.s};
        hipStream_t s = st.s;
        const size_t N = (size_t)n;

        std::vector<long long> h_off(N + 1, 0);
        if (dev) {
            HIP_CHECK(hipMemcpy(h_off.data(), run_offsets, (N + 1) * 8, hipMemcpyDeviceToHost));
            answer(rle_draw::check_run_offsets(reinterpret_cast<const int64_t*>(h_off.data()), n, who, &err), err);
        } else memcpy(h_off.data(), run_offsets, (N + 1) * 8);
        for (size_t k = 0; k < N; ++k)
            MRCNN_REQUIRE(h_off[k + 1] - h_off[k] < (1LL << 31), MRCNN_ERR_SHAPE, "rle_morph: RLE %lld has %lld runs: too many", (long long)k, h_off[k + 1] - h_off[k]);
        const size_t runs = (size_t)(h_off[N] - 0);
        MRCNN_REQUIRE(counts || h_off[N] == h_off[0], MRCNN_ERR_INVALID, "rle_morph: null counts");

        long long* ro = reinterpret_cast<long long*>(out_run_offsets);
        uint32_t* ar = areas;
        int32_t* bb = bboxes_xywh;
        if (!dev) {
            tro.alloc((N + 1) * sizeof(long long)); ro = tro.as<long long>();
            if (areas) { tar.alloc((N ? N : 1) * sizeof(uint32_t)); ar = tar.as<uint32_t>(); }
            if (bboxes_xywh) { tbb.alloc((N ? N : 1) * 4 * sizeof(int32_t)); bb = tbb.as<int32_t>(); }
        }
        if (n == 0) {
            HIP_CHECK(hipMemset(ro, 0, sizeof(long long)));
            if (!dev) out_run_offsets[0] = 0;
            return;
        }
        const uint32_t* c = counts;
        const long long* off = reinterpret_cast<const long long*>(run_offsets);
        if (!dev) {
            tc.alloc((runs ? runs : 1) * 4); to.alloc((N + 1) * 8);
            if (runs) HIP_CHECK(hipMemcpy(tc.p, counts, runs * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(to.p, h_off.data(), (N + 1) * 8, hipMemcpyHostToDevice));
            c = tc.as<uint32_t>(); off = to.as<long long>();
        }
        tp.alloc((runs ? runs : 1) * 4);
        // one scratch allocation: heights | widths | totals | areas | extents | the flag and the boxes (read back together) | records | segments | runs
        const auto s_h = sc.take<int32_t>(N), s_w = sc.take<int32_t>(N);
        const auto s_tot = sc.take<unsigned long long>(N);
        const auto s_ar = sc.take<uint32_t>(N);
        const auto s_ext = sc.take<uint2>(N);
        const auto s_bad = sc.take<unsigned long long>(2);       // (16 bytes: the boxes follow at once)
        const auto s_box = sc.take<MorphBox>(N);
        const auto s_rec = sc.take<MorphRec>(N);
        const auto s_seg = sc.take<RleSeg>(N * RLE_SEGS);
        const auto s_run = sc.take<uint32_t>(N);
        sc.alloc();
        HIP_CHECK(hipMemcpy(sc[s_h], heights, N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(sc[s_w], widths, N * 4, hipMemcpyHostToDevice));
        rle_prefix_forward(s, c, off, (long)n, tp.as<uint32_t>(), nullptr, sc[s_tot], sc[s_ar], sc[s_ext]);
        rle_morph_boxes_forward(s, c, tp.as<uint32_t>(), off, sc[s_h], sc[s_w], sc[s_tot], sc[s_ext], (long)n, sc[s_box], sc[s_bad]);
        static_assert(sizeof(MorphBox) == 16, "the flag's 16 bytes and the boxes are read back as one array");
        std::vector<MorphBox> got(N + 1);
        HIP_CHECK(hipMemcpyAsync(got.data(), sc[s_bad], (N + 1) * sizeof(MorphBox), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        unsigned long long k_bad;
        memcpy(&k_bad, got.data(), sizeof k_bad);
        if (k_bad != ~0ull) {                                    // the one flag said no: fetch the sum for the message
            unsigned long long sum = 0;
            HIP_CHECK(hipMemcpy(&sum, sc[s_tot] + k_bad, sizeof sum, hipMemcpyDeviceToHost));
            answer(rle_morph::bad_sum(a, (int64_t)k_bad, sum, who, &err), err);
        }

        // the layout of the call's bit boxes, columns and tiles from the boxes
        std::vector<MorphRec> rec(N);
        MorphJob job{};
        long long words = 0;
        for (size_t k = 0; k < N; ++k) {
            MorphRec& q = rec[k];
            q.r0 = h_off[k]; q.nruns = (int)(h_off[k + 1] - h_off[k]);
            q.h = heights[k]; q.w = widths[k]; q.r = radii[k]; q.pad = 0;
            q.tight = got[k + 1];
            q.work = morph_work_box(q.tight, q.r, q.h, q.w, morph_grows(op));
            const long long bw = q.work.x2 - q.work.x1, chunk = MORPH_TILE - 2 * q.r;
            q.words = (q.work.y2 - q.work.y1 + 31) / 32;
            q.word0 = words; q.col0 = job.cols; q.tile0 = job.tiles;
            words += bw * q.words; job.cols += bw; job.tiles += q.words * ((bw + chunk - 1) / chunk);
        }
        MRCNN_REQUIRE(job.tiles < (1LL << 31) && job.cols < (1LL << 39), MRCNN_ERR_SHAPE, "rle_morph: the set's boxes make %lld tiles: too many for one call", job.tiles);
        HIP_CHECK(hipMemcpyAsync(sc[s_rec], rec.data(), N * sizeof(MorphRec), hipMemcpyHostToDevice, s));
        bits.alloc((size_t)(words ? 2 * words : 1) * sizeof(uint32_t));
        job.rec = sc[s_rec]; job.n = (int)n; job.op = op;
        job.counts = c; job.pre_b = tp.as<uint32_t>();
        job.va = bits.as<uint32_t>(); job.vb = bits.as<uint32_t>() + words;
        rle_morph_forward(s, job);
        rle_morph_count_forward(s, job, sc[s_seg], sc[s_run], ro, ar, bb);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + N, sizeof(need), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(out_run_offsets, tro.p, (N + 1) * sizeof(long long), hipMemcpyDeviceToHost));
            if (areas) HIP_CHECK(hipMemcpy(areas, tar.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (bboxes_xywh) HIP_CHECK(hipMemcpy(bboxes_xywh, tbb.p, N * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        if (need > (long long)capacity) answer(rle_morph::bad_capacity(need, (long long)capacity, who, &err), err);
        uint32_t* oc = out_counts;
        if (!dev) { tcnt.alloc((size_t)need * sizeof(uint32_t)); oc = tcnt.as<uint32_t>(); }
        rle_morph_write_forward(s, job, sc[s_seg], ro, oc);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(out_counts, tcnt.p, (size_t)need * sizeof(uint32_t), hipMemcpyDeviceToHost));    // only the used part crosses PCIe
    });
}
