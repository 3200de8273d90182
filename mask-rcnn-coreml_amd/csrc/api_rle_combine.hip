// api_rle_combine.hip — the C ABI of include/maskrcnn_hip.h, combining run-length masks: union, intersection, symmetric difference and
// difference over caller-chosen groups of an RLE set — the host definition (rle_combine_host.cpp behind it) and the device entry
// (kernels_rle_combine.hip, with the boxes and the encoder of kernels_rle_morph.hip).  Every argument error is answered before a device
// is looked for.
#include <string.h>

#include "api_util.h"
#include "combine_rule.h"
#include "rle_combine_host.h"
#include "rle_draw_host.h"

using namespace mrcnn;

extern "C" int mrcnn_rle_combine_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                      const int64_t* group_offsets, const int64_t* members, int64_t n_groups, int op, uint32_t* out_counts,
                                      int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        std::string err;
        answer(rle_combine::combine_host(rle_combine::Set{counts, run_offsets, n, heights, widths, group_offsets, members, n_groups, op}, out_counts, capacity,
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
        const rle_combine::Set a{counts, run_offsets, n, heights, widths, group_offsets, members, n_groups, op};
        answer(rle_combine::check_arguments(a, out_counts, capacity, out_run_offsets, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_combine: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) {                                              // the offsets can be judged here: before a device is looked for
            answer(rle_draw::check_run_offsets(run_offsets, n, who, &err), err);
            MRCNN_REQUIRE(counts || run_offsets[n] == run_offsets[0], MRCNN_ERR_INVALID, "rle_combine: null counts");
        }
        require_gpu();
        Stream st;
        DevBuf tc, to, tp, tro, tar, tbb, tcnt, bits;
        Carver sc;
        Drain drain{st.s};
        hipStream_t s = st.s;
        const size_t N = (size_t)n, G = (size_t)n_groups, M = (size_t)group_offsets[n_groups];

        std::vector<long long> h_off(N + 1, 0);
        if (dev) {
            HIP_CHECK(hipMemcpy(h_off.data(), run_offsets, (N + 1) * 8, hipMemcpyDeviceToHost));
            answer(rle_draw::check_run_offsets(reinterpret_cast<const int64_t*>(h_off.data()), n, who, &err), err);
        } else memcpy(h_off.data(), run_offsets, (N + 1) * 8);
        for (size_t k = 0; k < N; ++k)
            MRCNN_REQUIRE(h_off[k + 1] - h_off[k] < (1LL << 31), MRCNN_ERR_SHAPE, "rle_combine: RLE %lld has %lld runs: too many", (long long)k, h_off[k + 1] - h_off[k]);
        const size_t runs = (size_t)h_off[N];
        MRCNN_REQUIRE(counts || h_off[N] == h_off[0], MRCNN_ERR_INVALID, "rle_combine: null counts");

        long long* ro = reinterpret_cast<long long*>(out_run_offsets);
        uint32_t* ar = areas;
        int32_t* bb = bboxes_xywh;
        if (!dev) {
            tro.alloc((G + 1) * sizeof(long long)); ro = tro.as<long long>();
            if (areas) { tar.alloc((G ? G : 1) * sizeof(uint32_t)); ar = tar.as<uint32_t>(); }
            if (bboxes_xywh) { tbb.alloc((G ? G : 1) * 4 * sizeof(int32_t)); bb = tbb.as<int32_t>(); }
        }
        auto nothing = [&] {                                     // no group: the offsets' one entry
            HIP_CHECK(hipMemset(ro, 0, sizeof(long long)));
            if (!dev) out_run_offsets[0] = 0;
        };
        if (n == 0) return nothing();                            // (and no group: a group needs a member)
        const uint32_t* c = counts;
        const long long* off = reinterpret_cast<const long long*>(run_offsets);
        if (!dev) {
            tc.alloc((runs ? runs : 1) * 4); to.alloc((N + 1) * 8);
            if (runs) HIP_CHECK(hipMemcpy(tc.p, counts, runs * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(to.p, h_off.data(), (N + 1) * 8, hipMemcpyHostToDevice));
            c = tc.as<uint32_t>(); off = to.as<long long>();
        }
        tp.alloc((runs ? runs : 1) * 4);
        // one scratch allocation: heights | widths | totals | areas | extents | the flag and the boxes (read back together) | the groups' records |
        // their first members | the members | segments | runs
        const auto s_h = sc.take<int32_t>(N), s_w = sc.take<int32_t>(N);
        const auto s_tot = sc.take<unsigned long long>(N);
        const auto s_ar = sc.take<uint32_t>(N);
        const auto s_ext = sc.take<uint2>(N);
        const auto s_bad = sc.take<unsigned long long>(2);       // (16 bytes: the boxes follow at once)
        const auto s_box = sc.take<MorphBox>(N);
        const auto s_rec = sc.take<MorphRec>(G);
        const auto s_m0 = sc.take<long long>(G + 1);
        const auto s_mem = sc.take<CombineMember>(M);
        const auto s_seg = sc.take<RleSeg>(G * RLE_SEGS);
        const auto s_run = sc.take<uint32_t>(G);
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
            answer(rle_combine::bad_sum(a, (int64_t)k_bad, sum, who, &err), err);
        }
        if (n_groups == 0) return nothing();

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
                mem[(size_t)j] = CombineMember{h_off[k], (int)(h_off[k + 1] - h_off[k]), got[k + 1], 0};
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
        job.counts = c; job.pre_b = tp.as<uint32_t>(); job.bits = bits.as<uint32_t>();
        rle_combine_forward(s, job);
        MorphJob enc{};                                          // the encoder of mrcnn_rle_morph on the groups' bit boxes
        enc.rec = sc[s_rec]; enc.n = (int)n_groups; enc.vb = bits.as<uint32_t>();
        rle_morph_count_forward(s, enc, sc[s_seg], sc[s_run], ro, ar, bb);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + G, sizeof(need), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(out_run_offsets, tro.p, (G + 1) * sizeof(long long), hipMemcpyDeviceToHost));
            if (areas) HIP_CHECK(hipMemcpy(areas, tar.p, G * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (bboxes_xywh) HIP_CHECK(hipMemcpy(bboxes_xywh, tbb.p, G * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        if (need > (long long)capacity) answer(rle_combine::bad_capacity(need, (long long)capacity, who, &err), err);
        uint32_t* oc = out_counts;
        if (!dev) { tcnt.alloc((size_t)need * sizeof(uint32_t)); oc = tcnt.as<uint32_t>(); }
        rle_morph_write_forward(s, enc, sc[s_seg], ro, oc);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(out_counts, tcnt.p, (size_t)need * sizeof(uint32_t), hipMemcpyDeviceToHost));    // only the used part crosses PCIe
    });
}
