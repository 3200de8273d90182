// api_rle_combine.hip — the C ABI of include/maskrcnn_hip.h, combining run-length masks: union, intersection, symmetric difference and
// difference over caller-chosen groups of an RLE set — the host definition (rle_combine_host.cpp behind it) and the device entry
// (kernels_rle_combine.hip, with the boxes and the encoder of kernels_rle_morph.hip).  Every argument error is answered before a device
// is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "combine_rule.h"
#include "rle_combine_host.h"

using namespace mrcnn;

extern "C" int mrcnn_rle_combine_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                      const int64_t* group_offsets, const int64_t* members, int64_t n_groups, int op, uint32_t* out_counts,
                                      int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(rle_combine::combine_host(rle_combine::Set{{counts, run_offsets, n, heights, widths}, group_offsets, members, n_groups, op}, out_counts, capacity,
                                         out_run_offsets, areas, bboxes_xywh, &err), err);
    });
}

extern "C" int mrcnn_rle_combine(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                 const int64_t* group_offsets, const int64_t* members, int64_t n_groups, int op, int memspace, uint32_t* out_counts,
                                 int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        const char* who = "rle_combine";
        std::string err;
        const rle_combine::Set a{{counts, run_offsets, n, heights, widths}, group_offsets, members, n_groups, op};
        answer(rle_combine::check_arguments(a, out_counts, capacity, out_run_offsets, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_combine: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);     // the offsets can be judged here: before a device is looked for
        require_gpu();
        Stream st;
        hipStream_t s = st.s;
        const size_t N = (size_t)n, G = (size_t)n_groups, M = (size_t)group_offsets[n_groups];
        DevBuf bits;
        Carver sc;
        StagedRle in(counts, run_offsets, n, dev, who);
        // one scratch allocation: the head's arrays | segments | runs | the groups' records | their first members | the members
        RleBoxes boxes(sc, N);
        RunsOut out(sc, G, dev, out_counts, capacity, out_run_offsets, areas, bboxes_xywh);
        const auto s_rec = sc.take<MorphRec>(G);
        const auto s_m0 = sc.take<long long>(G + 1);
        const auto s_mem = sc.take<CombineMember>(M);
        Drain drain{s};                                          // (declared behind the buffers: the stream drains before they are freed)
        if (n == 0) return out.nothing();                        // (and no group: a group needs a member)
        in.stage();
        sc.alloc();
        boxes.run(s, sc, in, a, who);
        if (n_groups == 0) return out.nothing();
        const std::vector<MorphBox>& got = boxes.got;

        // the work box of every group and the layout of the call's bit boxes and columns from the boxes read back; the member table
        std::vector<MorphRec> rec(G);
        std::vector<CombineMember> mem(M);
        CombineJob job{};
        long long words = 0;
        for (size_t g = 0; g < G; ++g) {
            MorphRec& q = rec[g];
            q = MorphRec{};
            const int64_t first = members[group_offsets[g]];
            q.h = heights[first]; q.w = widths[first];
            q.work = got[(size_t)first + 1];
            for (int64_t j = group_offsets[g]; j < group_offsets[g + 1]; ++j) {
                const size_t k = (size_t)members[j];
                mem[(size_t)j] = CombineMember{in.first(k), in.n_runs(k), got[k + 1], 0};
                if (!combine_in_first(op)) q.work = combine_hull(q.work, got[k + 1]);
            }
            q.tight = q.work;
            const long long bw = q.work.x2 - q.work.x1;
            q.words = (q.work.y2 - q.work.y1 + 31) / 32;
            q.word0 = words; q.col0 = job.cols;
            words += bw * q.words; job.cols += bw;
        }
        MRCNN_REQUIRE(job.cols < (1LL << 39), MRCNN_ERR_SHAPE, "rle_combine: the groups' boxes have %lld columns: too many for one call", job.cols);
        HIP_CHECK(hipMemcpyAsync(sc[s_rec], rec.data(), G * sizeof(MorphRec), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(sc[s_m0], group_offsets, (G + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(sc[s_mem], mem.data(), M * sizeof(CombineMember), hipMemcpyHostToDevice, s));
        bits.alloc((size_t)(words ? words : 1) * sizeof(uint32_t));
        job.rec = sc[s_rec]; job.n = (int)n_groups; job.member0 = sc[s_m0]; job.members = sc[s_mem]; job.op = op;
        job.counts = in.counts; job.pre_b = in.pre_b; job.bits = bits.as<uint32_t>();
        rle_combine_forward(s, job);
        MorphJob enc{};                                          // the encoder of mrcnn_rle_morph on the groups' bit boxes
        enc.rec = sc[s_rec]; enc.n = (int)n_groups; enc.vb = bits.as<uint32_t>();
        out.encode(s, sc, enc, who);
    });
}
