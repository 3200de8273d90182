// api_rle_morph.hip — the C ABI of include/maskrcnn_hip.h, changing run-length masks: erosion, dilation and the boundary band of an RLE
// set — the host definition (rle_morph_host.cpp behind it), the device entry (kernels_rle_morph.hip) and the radius Boundary IoU takes
// from an image's diagonal.  Every argument error is answered before a device is looked for.
#include <math.h>
#include <string.h>

#include "api_rle_stage.h"
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
        answer(rle_morph::morph_host(rle_morph::Set{{counts, run_offsets, n, heights, widths}, radii, op}, out_counts, capacity, out_run_offsets, areas,
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
        const rle_morph::Set a{{counts, run_offsets, n, heights, widths}, radii, op};
        answer(rle_morph::check_arguments(a, out_counts, capacity, out_run_offsets, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_morph: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);     // the offsets can be judged here: before a device is looked for
        require_gpu();
        Stream st;
        hipStream_t s = st.s;
        const size_t N = (size_t)n;
        DevBuf bits;
        Carver sc;
        StagedRle in(counts, run_offsets, n, dev, who);
        // one scratch allocation: the head's arrays | segments | runs | records
        RleBoxes boxes(sc, N);
        RunsOut out(sc, N, dev, out_counts, capacity, out_run_offsets, areas, bboxes_xywh);
        const auto s_rec = sc.take<MorphRec>(N);
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        if (n == 0) return out.nothing();
        in.stage();
        sc.alloc();
        boxes.run(s, sc, in, a, who);

        // the layout of the call's bit boxes, columns and tiles from the boxes
        std::vector<MorphRec> rec(N);
        MorphJob job{};
        long long words = 0;
        for (size_t k = 0; k < N; ++k) {
            MorphRec& q = rec[k];
            q.r0 = in.first(k); q.nruns = in.n_runs(k);
            q.h = heights[k]; q.w = widths[k]; q.r = radii[k]; q.pad = 0;
            q.tight = boxes.got[k + 1];
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
        job.counts = in.counts; job.pre_b = in.pre_b;
        job.va = bits.as<uint32_t>(); job.vb = bits.as<uint32_t>() + words;
        rle_morph_forward(s, job);
        out.encode(s, sc, job, who);
    });
}
