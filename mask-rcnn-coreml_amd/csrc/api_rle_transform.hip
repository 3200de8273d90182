// api_rle_transform.hip — the C ABI of include/maskrcnn_hip.h, moving run-length masks to another pixel grid: crop, place, flip,
// transpose, the rotations and nearest resizes of an RLE set under one rule — the host definition (rle_transform_host.cpp behind it)
// and the device entry (kernels_rle_transform.hip, with the boxes and the encoder of kernels_rle_morph.hip).  Every argument error is
// answered before a device is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "transform_rule.h"
#include "rle_transform_host.h"

using namespace mrcnn;

extern "C" int mrcnn_rle_transform_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                        const int32_t* out_heights, const int32_t* out_widths, const int64_t* xf, uint32_t* out_counts, int64_t capacity,
                                        int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(rle_transform::transform_host(rle_transform::Set{{counts, run_offsets, n, heights, widths}, out_heights, out_widths, xf}, out_counts, capacity,
                                             out_run_offsets, areas, bboxes_xywh, &err), err);
    });
}

extern "C" int mrcnn_rle_transform(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                   const int32_t* out_heights, const int32_t* out_widths, const int64_t* xf, int memspace, uint32_t* out_counts,
                                   int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        const char* who = "rle_transform";
        std::string err;
        const rle_transform::Set a{{counts, run_offsets, n, heights, widths}, out_heights, out_widths, xf};
        answer(rle_transform::check_arguments(a, out_counts, capacity, out_run_offsets, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_transform: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);     // the offsets can be judged here: before a device is looked for
        require_gpu();
        Stream st;
        hipStream_t s = st.s;
        const size_t N = (size_t)n;
        DevBuf bits;
        Carver sc;
        StagedRle in(counts, run_offsets, n, dev, who);
        // one scratch allocation: the head's arrays | segments | runs | the outputs' records | their sources
        RleBoxes boxes(sc, N);
        RunsOut out(sc, N, dev, out_counts, capacity, out_run_offsets, areas, bboxes_xywh);
        const auto s_rec = sc.take<MorphRec>(N);
        const auto s_src = sc.take<XfSource>(N);
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        if (n == 0) return out.nothing();
        in.stage();
        sc.alloc();
        boxes.run(s, sc, in, a, who);

        // the work box of every output — the preimage of the source's tight box, clipped to the output plane — and the layout of the
        // call's bit boxes and columns
        std::vector<MorphRec> rec(N);
        std::vector<XfSource> src(N);
        XfJob job{};
        long long words = 0;
        for (size_t k = 0; k < N; ++k) {
            XfSource& e = src[k];
            e = XfSource{in.first(k), in.n_runs(k), heights[k], widths[k], 0, boxes.got[k + 1], xf_map(xf + 8 * k)};
            MorphRec& q = rec[k];
            q = MorphRec{};
            q.h = out_heights[k]; q.w = out_widths[k];
            q.work = xf_work_box(e.map, e.tight, q.h, q.w);
            q.tight = q.work;
            const long long bw = q.work.x2 - q.work.x1;
            q.words = (q.work.y2 - q.work.y1 + 31) / 32;
            q.word0 = words; q.col0 = job.cols;
            words += bw * q.words; job.cols += bw;
        }
        MRCNN_REQUIRE(words <= MRCNN_XF_MAX_BOX_WORDS, MRCNN_ERR_SHAPE,
                      "rle_transform: the results' boxes take %lld words of bits, more than MRCNN_XF_MAX_BOX_WORDS = %lld: split the set", words,
                      (long long)MRCNN_XF_MAX_BOX_WORDS);
        HIP_CHECK(hipMemcpyAsync(sc[s_rec], rec.data(), N * sizeof(MorphRec), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(sc[s_src], src.data(), N * sizeof(XfSource), hipMemcpyHostToDevice, s));
        bits.alloc((size_t)(words ? words : 1) * sizeof(uint32_t));
        job.rec = sc[s_rec]; job.n = (int)n; job.src = sc[s_src];
        job.counts = in.counts; job.pre_b = in.pre_b; job.bits = bits.as<uint32_t>();
        rle_transform_forward(s, job);
        MorphJob enc{};                                          // the encoder of mrcnn_rle_morph on the bit boxes
        enc.rec = sc[s_rec]; enc.n = (int)n; enc.vb = bits.as<uint32_t>();
        out.encode(s, sc, enc, who);
    });
}
