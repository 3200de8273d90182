// api_rle_stage.h — what the device entries of the run-length mask families share (api_rle_*.hip, api_polygons.hip): the staging of an
// RLE set on the device (rle_set_host.h is its host rule), the one read-back of the flag that refuses an RLE which does not sum to its
// plane, and the head and the tail mrcnn_rle_morph and mrcnn_rle_combine have in common.  Header-only; internal linkage, nothing here is
// exported.
#pragma once
#include <string.h>

#include "api_util.h"
#include "rle_set_host.h"

namespace mrcnn {

// The runs of an RLE set for the kernels.  The constructor brings run_offsets to the host and judges them — an entry may still answer
// an empty set after it without an allocation — and stage() puts the set on the device: the caller's own arrays for MRCNN_DEVICE,
// otherwise an upload; and the prefix table rle_prefix_forward fills.  Declare it before the stream's Drain: the buffers outlive the
// queued work.
struct StagedRle {
    std::vector<long long> h_off;            // run_offsets on the host, n + 1
    long long runs = 0;                      // the runs of the set: h_off[n] - h_off[0]
    const uint32_t* counts;                  // on the device after stage()
    const long long* run_offsets;
    uint32_t* pre_b = nullptr;               // one entry per count up to the last RLE's end
    const bool dev;
    DevBuf tc, to, tp;

    long long first(size_t k) const { return h_off[k]; }                         // RLE k's first run and how many it has
    int n_runs(size_t k) const { return (int)(h_off[k + 1] - h_off[k]); }

    // The half that needs no device, for a set in host memory: an entry runs it before it looks for one.  counts may be null exactly
    // when the set has no runs.
    static void check_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const char* who)
    {
        std::string err;
        answer(rle_set::check_run_offsets(run_offsets, n, who, &err), err);
        answer(rle_set::check_counts(counts, run_offsets, n, who, &err), err);
    }

    StagedRle(const uint32_t* c, const int64_t* off, int64_t n, bool on_device, const char* who)
        : h_off((size_t)n + 1, 0), counts(c), run_offsets(reinterpret_cast<const long long*>(off)), dev(on_device)
    {
        const size_t N = (size_t)n;
        if (dev) HIP_CHECK(hipMemcpy(h_off.data(), off, (N + 1) * 8, hipMemcpyDeviceToHost));
        else memcpy(h_off.data(), off, (N + 1) * 8);
        const int64_t* judged = reinterpret_cast<const int64_t*>(h_off.data());
        std::string err;
        answer(rle_set::check_run_offsets(judged, n, who, &err), err);
        for (size_t k = 0; k < N; ++k)
            MRCNN_REQUIRE(h_off[k + 1] - h_off[k] < (1LL << 31), MRCNN_ERR_SHAPE, "%s: RLE %lld has %lld runs: too many", who, (long long)k, h_off[k + 1] - h_off[k]);
        answer(rle_set::check_counts(c, judged, n, who, &err), err);
        runs = h_off[N] - h_off[0];
    }

    void stage()
    {
        const size_t N = h_off.size() - 1, upto = (size_t)h_off[N];      // all of counts up to the last RLE's end: the offsets hold as they are
        if (!dev) {
            tc.alloc((upto ? upto : 1) * 4); to.alloc((N + 1) * 8);
            if (counts && upto) HIP_CHECK(hipMemcpy(tc.p, counts, upto * 4, hipMemcpyHostToDevice));   // (null counts: no runs, nothing to copy)
            HIP_CHECK(hipMemcpy(to.p, h_off.data(), (N + 1) * 8, hipMemcpyHostToDevice));
            counts = tc.as<uint32_t>(); run_offsets = to.as<long long>();
        }
        tp.alloc((upto ? upto : 1) * 4);
        pre_b = tp.as<uint32_t>();
    }
};

// The one read-back before anything is written.  The first word at `flag` is the lowest RLE that does not sum to its plane, ~0 for none;
// an entry that laid out more behind it reads that in the same copy (`bytes` into `into`).  Returns after the synchronise; when an RLE
// was refused, with its sum fetched from `totals` for the message (bad_sum of rle_set_host.h or rle_draw_host.h).
struct Refusal { bool any; int64_t k; unsigned long long sum; };
static Refusal read_refusal(hipStream_t s, const void* flag, const unsigned long long* totals, void* into = nullptr, size_t bytes = 0)
{
    unsigned long long k = ~0ull;
    if (!into) { into = &k; bytes = sizeof k; }
    HIP_CHECK(hipMemcpyAsync(into, flag, bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    memcpy(&k, into, sizeof k);
    Refusal r{k != ~0ull, (int64_t)k, 0};
    if (r.any) HIP_CHECK(hipMemcpy(&r.sum, totals + k, sizeof r.sum, hipMemcpyDeviceToHost));
    return r;
}

// The head of mrcnn_rle_morph and mrcnn_rle_combine: heights and widths on the device, the prefix table and the tight box of every RLE,
// read back with the flag in one copy.  Its arrays are carved from the entry's one scratch allocation: construct it, take the entry's
// own slots, sc.alloc(), then run().
struct RleBoxes {
    const Carver::Slot<int32_t> h, w;
    const Carver::Slot<unsigned long long> tot;
    const Carver::Slot<uint32_t> ar;
    const Carver::Slot<uint2> ext;
    const Carver::Slot<unsigned long long> bad;                  // (16 bytes: the boxes follow at once)
    const Carver::Slot<MorphBox> box;
    std::vector<MorphBox> got;                                   // got[k + 1] is RLE k's box; got[0] the flag's 16 bytes

    RleBoxes(Carver& sc, size_t N)
        : h(sc.take<int32_t>(N)), w(sc.take<int32_t>(N)), tot(sc.take<unsigned long long>(N)), ar(sc.take<uint32_t>(N)), ext(sc.take<uint2>(N)),
          bad(sc.take<unsigned long long>(2)), box(sc.take<MorphBox>(N)), got(N + 1)
    {
        static_assert(sizeof(MorphBox) == 16, "the flag's 16 bytes and the boxes are read back as one array");
    }

    void run(hipStream_t s, const Carver& sc, const StagedRle& in, const rle_set::Flat& a, const char* who)
    {
        const size_t N = got.size() - 1;
        HIP_CHECK(hipMemcpy(sc[h], a.heights, N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(sc[w], a.widths, N * 4, hipMemcpyHostToDevice));
        rle_prefix_forward(s, in.counts, in.run_offsets, (long)a.n, in.pre_b, nullptr, sc[tot], sc[ar], sc[ext]);
        rle_morph_boxes_forward(s, in.counts, in.pre_b, in.run_offsets, sc[h], sc[w], sc[tot], sc[ext], (long)a.n, sc[box], sc[bad]);
        const Refusal r = read_refusal(s, sc[bad], sc[tot], got.data(), (N + 1) * sizeof(MorphBox));
        std::string err;
        if (r.any) answer(rle_set::bad_sum(a, r.k, r.sum, who, &err), err);
    }
};

// The tail of both: the bit boxes of G records (a MorphJob's rec, n and vb) encoded into the caller's RLE outputs.  The constructor
// stages out_run_offsets, areas and bboxes_xywh for a host caller and takes the encoder's scratch from the entry's allocation.  Declare
// it before the stream's Drain.
struct RunsOut {
    const bool dev;
    const size_t G;
    uint32_t* const out_counts; const int64_t capacity; int64_t* const out_run_offsets; uint32_t* const areas; int32_t* const bboxes_xywh;
    long long* ro; uint32_t* ar; int32_t* bb;                    // where the kernels write
    DevBuf tro, tar, tbb, tcnt;
    const Carver::Slot<RleSeg> seg;
    const Carver::Slot<uint32_t> run;

    RunsOut(Carver& sc, size_t groups, bool on_device, uint32_t* counts_out, int64_t cap, int64_t* offsets_out, uint32_t* areas_out, int32_t* boxes_out)
        : dev(on_device), G(groups), out_counts(counts_out), capacity(cap), out_run_offsets(offsets_out), areas(areas_out), bboxes_xywh(boxes_out),
          ro(reinterpret_cast<long long*>(offsets_out)), ar(areas_out), bb(boxes_out), seg(sc.take<RleSeg>(groups * RLE_SEGS)), run(sc.take<uint32_t>(groups))
    {
        if (dev) return;
        tro.alloc((G + 1) * sizeof(long long)); ro = tro.as<long long>();
        if (areas) { tar.alloc((G ? G : 1) * sizeof(uint32_t)); ar = tar.as<uint32_t>(); }
        if (bboxes_xywh) { tbb.alloc((G ? G : 1) * 4 * sizeof(int32_t)); bb = tbb.as<int32_t>(); }
    }

    // no record: the offsets' one entry
    void nothing()
    {
        HIP_CHECK(hipMemset(ro, 0, sizeof(long long)));
        if (!dev) out_run_offsets[0] = 0;
    }

    void encode(hipStream_t s, const Carver& sc, const MorphJob& job, const char* who)
    {
        rle_morph_count_forward(s, job, sc[seg], sc[run], ro, ar, bb);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + G, sizeof(need), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(out_run_offsets, tro.p, (G + 1) * sizeof(long long), hipMemcpyDeviceToHost));
            if (areas) HIP_CHECK(hipMemcpy(areas, tar.p, G * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (bboxes_xywh) HIP_CHECK(hipMemcpy(bboxes_xywh, tbb.p, G * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        std::string err;
        if (need > (long long)capacity) answer(rle_set::bad_runs_capacity(need, (long long)capacity, who, &err), err);
        uint32_t* oc = out_counts;
        if (!dev) { tcnt.alloc((size_t)need * sizeof(uint32_t)); oc = tcnt.as<uint32_t>(); }
        rle_morph_write_forward(s, job, sc[seg], ro, oc);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) HIP_CHECK(hipMemcpy(out_counts, tcnt.p, (size_t)need * sizeof(uint32_t), hipMemcpyDeviceToHost));    // only the used part crosses PCIe
    }
};

}  // namespace mrcnn
