// api_rle_components.hip — the C ABI of include/maskrcnn_hip.h, cutting run-length masks into their connected components: the host
// definitions (rle_components_host.cpp behind them) and the device entries (kernels_rle_components.hip) that label and measure, and
// that merge or split by a keep mask.  Every argument error is answered before a device is looked for.
#include <string.h>

#include "api_rle_stage.h"
#include "rle_components_host.h"

using namespace mrcnn;
namespace rc = mrcnn::rle_components;

extern "C" int mrcnn_rle_components_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                         int connectivity, int of, int64_t* comp_offsets, uint32_t* comp_areas, int32_t* comp_bboxes_xywh,
                                         uint8_t* comp_flags, int64_t comp_capacity)
{
    return guarded([&] {
        std::string err;
        answer(rc::components_host(rc::Set{{counts, run_offsets, n, heights, widths}, connectivity, of},
                                   rc::Measures{comp_offsets, comp_areas, comp_bboxes_xywh, comp_flags, comp_capacity}, &err), err);
    });
}

extern "C" int mrcnn_rle_components_select_host(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights,
                                                const int32_t* widths, int connectivity, int of, const uint8_t* keep, int64_t n_comps, int mode,
                                                uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh,
                                                int64_t* out_parent, int64_t* out_n)
{
    return guarded([&] {
        std::string err;
        answer(rc::select_host(rc::Set{{counts, run_offsets, n, heights, widths}, connectivity, of},
                               rc::Select{keep, n_comps, mode, out_counts, capacity, out_run_offsets, areas, bboxes_xywh, out_parent, out_n}, &err), err);
    });
}

namespace {

// The set on the device, labelled: what both device entries do first.  Declared before the stream's Drain in the caller: the buffers
// outlive the queued work.
struct Labelled {
    StagedRle in;
    Carver sc, pc;
    CompSet S{};
    CompPieces P{};
    long long* piece0 = nullptr;
    int32_t* comp_rle = nullptr;
    long long* comp_offsets = nullptr;       // device, n + 1
    long long n_comps = 0;
    Labelled(const rc::Set& a, bool dev, const char* who) : in(a.counts, a.run_offsets, a.n, dev, who) {}
};

void label(hipStream_t s, const rc::Set& a, const char* who, Labelled& L)
{
    std::string err;
    const size_t N = (size_t)a.n;
    const long long runs = L.in.runs;
    MRCNN_REQUIRE(runs < (1LL << 31), MRCNN_ERR_SHAPE, "%s: the set has %lld runs: too many for one call", who, runs);
    L.in.stage();
    const uint32_t* c = L.in.counts;
    const long long* off = L.in.run_offsets;
    // one scratch allocation: heights | widths | totals | areas | the flag and the number of pieces | pieces per run and their prefix | offsets
    Carver& sc = L.sc;
    const auto s_h = sc.take<int32_t>(N), s_w = sc.take<int32_t>(N);
    const auto s_tot = sc.take<unsigned long long>(N);
    const auto s_ar = sc.take<uint32_t>(N);
    const auto s_bad = sc.take<unsigned long long>(1);
    const auto s_cnt = sc.take<uint32_t>((size_t)runs + 1);
    const auto s_start = sc.take<unsigned long long>((size_t)runs + 1);
    const auto s_p0 = sc.take<long long>(N + 1);
    const auto s_co = sc.take<long long>(N + 1);
    sc.alloc();
    if (N) {
        HIP_CHECK(hipMemcpy(sc[s_h], a.heights, N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(sc[s_w], a.widths, N * 4, hipMemcpyHostToDevice));
    }
    rle_prefix_forward(s, c, off, (long)a.n, L.in.pre_b, nullptr, sc[s_tot], sc[s_ar]);
    CompSet& S = L.S;
    S.counts = c; S.pre_b = L.in.pre_b; S.run_offsets = off; S.heights = sc[s_h]; S.widths = sc[s_w]; S.totals = sc[s_tot];
    S.n = (int)a.n; S.connectivity = a.connectivity; S.of = a.of;
    rle_components_count_forward(s, S, runs, sc[s_cnt], sc[s_start], sc[s_bad]);
    unsigned long long n_pieces = 0;                         // read back with the flag: one synchronise
    HIP_CHECK(hipMemcpyAsync(&n_pieces, sc[s_start] + runs, 8, hipMemcpyDeviceToHost, s));
    const Refusal r = read_refusal(s, sc[s_bad], sc[s_tot]);
    if (r.any) answer(rle_set::bad_sum(a, r.k, r.sum, who, &err), err);
    MRCNN_REQUIRE(n_pieces < (1ull << 31), MRCNN_ERR_SHAPE, "%s: the set cuts into %llu column pieces: too many for one call", who, n_pieces);

    // the pieces: starts | ends | RLEs | parents | roots | numbers | root flags | their prefix | the components' RLEs
    const size_t Pn = (size_t)n_pieces, P1 = Pn ? Pn : 1;
    Carver& pc = L.pc;
    const auto p_a = pc.take<uint32_t>(P1), p_b = pc.take<uint32_t>(P1), p_par = pc.take<uint32_t>(P1), p_root = pc.take<uint32_t>(P1),
               p_comp = pc.take<uint32_t>(P1), p_isr = pc.take<uint32_t>(P1);
    const auto p_rle = pc.take<int32_t>(P1), p_crle = pc.take<int32_t>(P1);
    const auto p_cs = pc.take<unsigned long long>(Pn + 1);
    pc.alloc();
    L.P = CompPieces{(long long)Pn, pc[p_a], pc[p_b], pc[p_rle], pc[p_par], pc[p_root], pc[p_comp]};
    L.piece0 = sc[s_p0]; L.comp_rle = pc[p_crle]; L.comp_offsets = sc[s_co];
    rle_components_label_forward(s, S, runs, sc[s_start], L.P, L.piece0, pc[p_isr], pc[p_cs], L.comp_rle, L.comp_offsets);
    unsigned long long found = 0;
    HIP_CHECK(hipMemcpyAsync(&found, pc[p_cs] + Pn, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    L.n_comps = (long long)found;
}

}  // namespace

extern "C" int mrcnn_rle_components(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                    int connectivity, int of, int memspace, int64_t* comp_offsets, uint32_t* comp_areas, int32_t* comp_bboxes_xywh,
                                    uint8_t* comp_flags, int64_t comp_capacity)
{
    return guarded([&] {
        const char* who = "rle_components";
        std::string err;
        const rc::Set a{{counts, run_offsets, n, heights, widths}, connectivity, of};
        answer(rc::check_measures(a, rc::Measures{comp_offsets, comp_areas, comp_bboxes_xywh, comp_flags, comp_capacity}, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_components: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);     // the offsets can be judged here: before a device is looked for
        require_gpu();
        Stream st;
        Labelled L(a, dev, who);
        DevBuf tar, tbb, tfl;
        Carver ac;
        Drain drain{st.s};
        hipStream_t s = st.s;
        label(s, a, who, L);
        const size_t N = (size_t)n;
        HIP_CHECK(hipMemcpy(comp_offsets, L.comp_offsets, (N + 1) * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        // comp_offsets is written by now; the measures only when all components fit
        if (L.n_comps > (long long)comp_capacity) answer(rc::bad_comp_capacity(L.n_comps, (long long)comp_capacity, who, &err), err);
        if (L.n_comps == 0) return;
        const size_t C = (size_t)L.n_comps;
        uint32_t* ar = comp_areas; int32_t* bb = comp_bboxes_xywh; uint8_t* fl = comp_flags;
        if (!dev) {
            tar.alloc(C * 4); tbb.alloc(C * 16); tfl.alloc(C);
            ar = tar.as<uint32_t>(); bb = tbb.as<int32_t>(); fl = tfl.as<uint8_t>();
        }
        const auto c_ar = ac.take<uint32_t>(C), c_fl = ac.take<uint32_t>(C);
        const auto c_x1 = ac.take<int32_t>(C), c_y1 = ac.take<int32_t>(C), c_x2 = ac.take<int32_t>(C), c_y2 = ac.take<int32_t>(C);
        ac.alloc();
        rle_components_measure_forward(s, L.S, L.P, CompAcc{ac[c_ar], ac[c_x1], ac[c_y1], ac[c_x2], ac[c_y2], ac[c_fl]}, L.n_comps, ar, bb, fl);
        HIP_CHECK(hipStreamSynchronize(s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(comp_areas, tar.p, C * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(comp_bboxes_xywh, tbb.p, C * 16, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(comp_flags, tfl.p, C, hipMemcpyDeviceToHost));
        }
    });
}

extern "C" int mrcnn_rle_components_select(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* heights, const int32_t* widths,
                                           int connectivity, int of, const uint8_t* keep, int64_t n_comps, int mode, int memspace,
                                           uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh,
                                           int64_t* out_parent, int64_t* out_n)
{
    return guarded([&] {
        const char* who = "rle_components_select";
        std::string err;
        const rc::Set a{{counts, run_offsets, n, heights, widths}, connectivity, of};
        answer(rc::check_select(a, rc::Select{keep, n_comps, mode, out_counts, capacity, out_run_offsets, areas, bboxes_xywh, out_parent, out_n}, who, &err), err);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_components_select: unknown memspace %d", memspace);
        const bool dev = memspace == MRCNN_DEVICE;
        if (!dev) StagedRle::check_host(counts, run_offsets, n, who);
        require_gpu();
        Stream st;
        Labelled L(a, dev, who);
        DevBuf tkeep, tro, tar, tbb, tpar, tcnt, keys, bnd;
        Carver wc, gc;
        Drain drain{st.s};
        hipStream_t s = st.s;
        label(s, a, who, L);
        if (L.n_comps != (long long)n_comps) answer(rc::bad_n_comps((long long)n_comps, L.n_comps, who, &err), err);

        const bool split = mode == MRCNN_COMPONENTS_SPLIT;
        const size_t C = (size_t)n_comps, Pn = (size_t)L.P.n;
        const uint8_t* kp = keep;
        if (!dev && C) { tkeep.alloc(C); HIP_CHECK(hipMemcpy(tkeep.p, keep, C, hipMemcpyHostToDevice)); kp = tkeep.as<uint8_t>(); }
        // the selection's scratch: keep flags and their prefix | SPLIT's order and first places | boundaries per place and their prefix
        const auto w_kf = wc.take<uint32_t>(C + 1);
        const auto w_oi = wc.take<unsigned long long>(C + 1);
        const auto w_ord = wc.take<uint32_t>(Pn + 1);
        const auto w_cf = wc.take<long long>(C + 1);
        const auto w_bc = wc.take<uint32_t>(Pn + 1);
        const auto w_bp = wc.take<unsigned long long>(Pn + 1);
        // (the groups are sized below, once SPLIT knows how many components are kept)
        wc.alloc();
        CompSelect q{kp, (long long)n_comps, nullptr, nullptr, nullptr};
        long long G = (long long)n;
        if (split) {
            rle_components_keep_forward(s, kp, (long long)n_comps, wc[w_kf], wc[w_oi]);
            unsigned long long kept = 0;
            HIP_CHECK(hipMemcpyAsync(&kept, wc[w_oi] + C, 8, hipMemcpyDeviceToHost, s));
            keys.alloc((size_t)rle_components_sort_padded(L.P.n) * 8);
            rle_components_sort_forward(s, L.P, (long long)n_comps, keys.as<unsigned long long>(), wc[w_ord], wc[w_cf]);
            HIP_CHECK(hipStreamSynchronize(s));
            G = (long long)kept;
            q.order = wc[w_ord]; q.comp_first = wc[w_cf]; q.out_index = wc[w_oi];
        }
        const size_t Gn = (size_t)G, G1 = Gn ? Gn : 1;
        const auto g_b = gc.take<long long>(G1), g_e = gc.take<long long>(G1);
        const auto g_rle = gc.take<int32_t>(G1), g_x1 = gc.take<int32_t>(G1), g_y1 = gc.take<int32_t>(G1), g_x2 = gc.take<int32_t>(G1), g_y2 = gc.take<int32_t>(G1);
        const auto g_lead = gc.take<uint32_t>(G1), g_nr = gc.take<uint32_t>(G1), g_ar = gc.take<uint32_t>(G1);
        gc.alloc();
        const CompGroups grp{G, gc[g_b], gc[g_e], gc[g_rle], gc[g_lead], gc[g_nr], gc[g_ar], gc[g_x1], gc[g_y1], gc[g_x2], gc[g_y2]};

        long long* ro = reinterpret_cast<long long*>(out_run_offsets);
        long long* par = reinterpret_cast<long long*>(out_parent);
        uint32_t* ar = areas;
        int32_t* bb = bboxes_xywh;
        if (!dev) {
            tro.alloc((Gn + 1) * 8); ro = tro.as<long long>();
            if (out_parent) { tpar.alloc(G1 * 8); par = tpar.as<long long>(); }
            if (areas) { tar.alloc(G1 * 4); ar = tar.as<uint32_t>(); }
            if (bboxes_xywh) { tbb.alloc(G1 * 16); bb = tbb.as<int32_t>(); }
        }
        rle_components_groups_forward(s, L.S, L.P, q, L.piece0, L.comp_rle, grp, wc[w_bc], wc[w_bp], par, ro);
        long long need = 0;
        unsigned long long n_bnd = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + Gn, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&n_bnd, wc[w_bp] + Pn, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const bool fits = need <= (long long)capacity;
        uint32_t* oc = fits ? out_counts : nullptr;
        if (fits && !dev) { tcnt.alloc((size_t)(need ? need : 1) * 4); oc = tcnt.as<uint32_t>(); }
        bnd.alloc((size_t)(n_bnd ? n_bnd : 1) * 4);
        if (fits || areas || bboxes_xywh)
            rle_components_write_forward(s, L.S, L.P, q, grp, wc[w_bp], bnd.as<uint32_t>(), ro, need, oc, ar, bb);
        HIP_CHECK(hipStreamSynchronize(s));
        *out_n = (int64_t)G;                                     // (a host word in both memory spaces)
        if (!dev) {
            HIP_CHECK(hipMemcpy(out_run_offsets, tro.p, (Gn + 1) * 8, hipMemcpyDeviceToHost));
            if (out_parent && Gn) HIP_CHECK(hipMemcpy(out_parent, tpar.p, Gn * 8, hipMemcpyDeviceToHost));
            if (areas && Gn) HIP_CHECK(hipMemcpy(areas, tar.p, Gn * 4, hipMemcpyDeviceToHost));
            if (bboxes_xywh && Gn) HIP_CHECK(hipMemcpy(bboxes_xywh, tbb.p, Gn * 16, hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        if (!fits) answer(rle_set::bad_runs_capacity(need, (long long)capacity, who, &err), err);
        if (!dev && need) HIP_CHECK(hipMemcpy(out_counts, tcnt.p, (size_t)need * 4, hipMemcpyDeviceToHost));
    });
}
