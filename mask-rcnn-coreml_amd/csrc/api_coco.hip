// api_coco.hip — the C ABI of include/maskrcnn_hip.h, COCO scoring: mask / box IoU per image, COCOeval's matching
// (kernels_coco.hip), its accumulate (kernels_coco_acc.hip) and polygons to run-length masks: one annotation on the host, a whole
// annotation file on the device.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "api_util.h"

using namespace mrcnn;

// ================================================================================================
// COCO scoring (kernels_coco.hip): mask / box IoU per image and COCOeval's matching on the device
// ================================================================================================
namespace {

// an RLE set on the device with its prefix tables; `n` RLEs, run offsets validated on the host
struct RleSet {
    DevBuf counts_tmp, off_tmp, pre_b, pre_o, totals, areas;
    const uint32_t* counts = nullptr;
    const long long* off = nullptr;
    std::vector<long long> h_off;
    std::vector<unsigned long long> h_tot;
    void prepare(hipStream_t s, const char* what, const uint32_t* c, const int64_t* ro, int64_t n, int memspace, bool want_o)
    {
        h_off.assign((size_t)n + 1, 0);
        const bool dev = memspace == MRCNN_DEVICE;
        if (dev) HIP_CHECK(hipMemcpy(h_off.data(), ro, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
        else memcpy(h_off.data(), ro, (size_t)(n + 1) * 8);
        MRCNN_REQUIRE(h_off[0] >= 0, MRCNN_ERR_SHAPE, "rle_iou: %s run_offsets[0] = %lld is negative", what, h_off[0]);
        for (int64_t k = 0; k < n; ++k)
            MRCNN_REQUIRE(h_off[(size_t)k + 1] >= h_off[(size_t)k], MRCNN_ERR_SHAPE, "rle_iou: %s run_offsets decrease at RLE %lld", what, (long long)k);
        const size_t runs = (size_t)h_off[(size_t)n];
        MRCNN_REQUIRE(c || runs == 0, MRCNN_ERR_INVALID, "rle_iou: null %s counts", what);
        if (dev) { counts = c; off = reinterpret_cast<const long long*>(ro); }
        else {
            counts_tmp.alloc(runs * 4); off_tmp.alloc((size_t)(n + 1) * 8);
            if (runs) HIP_CHECK(hipMemcpy(counts_tmp.p, c, runs * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(off_tmp.p, h_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
            counts = counts_tmp.as<uint32_t>(); off = off_tmp.as<long long>();
        }
        pre_b.alloc(runs * 4);
        if (want_o) pre_o.alloc(runs * 4);
        totals.alloc((size_t)n * 8); areas.alloc((size_t)n * 4);
        rle_prefix_forward(s, counts, off, (long)n, pre_b.as<uint32_t>(), want_o ? pre_o.as<uint32_t>() : nullptr, totals.as<unsigned long long>(),
                           areas.as<uint32_t>());
        h_tot.assign((size_t)n, 0);
        HIP_CHECK(hipStreamSynchronize(s));
        if (n) HIP_CHECK(hipMemcpy(h_tot.data(), totals.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < n; ++k)
            MRCNN_REQUIRE(h_tot[(size_t)k] < (1ULL << 31), MRCNN_ERR_SHAPE, "rle_iou: %s RLE %lld sums to %llu pixels: more than a 32767 x 32767 plane", what,
                          (long long)k, h_tot[(size_t)k]);
    }
};

// checks the group table against the set sizes and the output capacity (blocks inside, no two overlapping); returns the pairs
long long check_iou_groups(const char* who, const mrcnn_iou_group* groups, int n_groups, int64_t n_d, int64_t n_g, int64_t n_pairs)
{
    MRCNN_REQUIRE(n_groups >= 0 && (groups || n_groups == 0) && n_d >= 0 && n_g >= 0 && n_pairs >= 0, MRCNN_ERR_INVALID, "bad %s argument", who);
    std::vector<std::pair<long long, long long>> blocks;
    long long pairs = 0;
    for (int k = 0; k < n_groups; ++k) {
        const mrcnn_iou_group& G = groups[k];
        MRCNN_REQUIRE(0 <= G.d0 && G.d0 <= G.d1 && G.d1 <= n_d && 0 <= G.g0 && G.g0 <= G.g1 && G.g1 <= n_g, MRCNN_ERR_SHAPE,
                      "%s: group %d names detections [%lld, %lld) of %lld and ground truths [%lld, %lld) of %lld", who, k, (long long)G.d0, (long long)G.d1,
                      (long long)n_d, (long long)G.g0, (long long)G.g1, (long long)n_g);
        const long long sz = (long long)(G.d1 - G.d0) * (G.g1 - G.g0);
        MRCNN_REQUIRE(G.out_offset >= 0 && G.out_offset + sz <= n_pairs, MRCNN_ERR_SHAPE, "%s: the block of group %d (%lld entries at %lld) leaves the %lld output entries",
                      who, k, sz, (long long)G.out_offset, (long long)n_pairs);
        if (sz) blocks.emplace_back((long long)G.out_offset, (long long)G.out_offset + sz);
        pairs += sz;
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t i = 1; i < blocks.size(); ++i)
        MRCNN_REQUIRE(blocks[i].first >= blocks[i - 1].second, MRCNN_ERR_SHAPE, "%s: two groups' output blocks overlap at entry %lld", who, blocks[i].first);
    return pairs;
}

// host results: only the entries a block covers are copied
template <class T>
void copy_blocks_to_host(T* dst, const T* dev, const mrcnn_iou_group* groups, int n_groups)
{
    for (int k = 0; k < n_groups; ++k) {
        const size_t sz = (size_t)(groups[k].d1 - groups[k].d0) * (size_t)(groups[k].g1 - groups[k].g0);
        if (sz) HIP_CHECK(hipMemcpy(dst + groups[k].out_offset, dev + groups[k].out_offset, sz * sizeof(T), hipMemcpyDeviceToHost));
    }
}

// the group table and `starts`, the prefix of the groups' work items, for the IoU kernels
void upload_groups(DevBuf& tab, DevBuf& st, const mrcnn_iou_group* groups, int n_groups, const std::vector<long long>& starts)
{
    tab.alloc((size_t)n_groups * sizeof(mrcnn_iou_group)); st.alloc(starts.size() * 8);
    HIP_CHECK(hipMemcpy(tab.p, groups, (size_t)n_groups * sizeof(mrcnn_iou_group), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(st.p, starts.data(), starts.size() * 8, hipMemcpyHostToDevice));
}

void upload_crowd(DevBuf& buf, const uint8_t* g_iscrowd, int64_t n_g)
{
    std::vector<uint8_t> c((size_t)(n_g > 0 ? n_g : 1), 0);
    if (g_iscrowd) for (int64_t i = 0; i < n_g; ++i) c[(size_t)i] = g_iscrowd[i] ? 1 : 0;
    buf.alloc(c.size());
    HIP_CHECK(hipMemcpy(buf.p, c.data(), c.size(), hipMemcpyHostToDevice));
}

}  // namespace

extern "C" int mrcnn_rle_iou(const uint32_t* d_counts, const int64_t* d_run_offsets, int64_t n_d, const uint32_t* g_counts,
                             const int64_t* g_run_offsets, int64_t n_g, const uint8_t* g_iscrowd, const mrcnn_iou_group* groups, int n_groups,
                             int memspace, uint32_t* inter, double* iou, int64_t n_pairs)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(d_run_offsets && g_run_offsets, MRCNN_ERR_INVALID, "rle_iou: null run offsets");
        const long long pairs = check_iou_groups("rle_iou", groups, n_groups, n_d, n_g, n_pairs);
        Stream st;
        RleSet D, G;
        D.prepare(st.s, "detection", d_counts, d_run_offsets, n_d, memspace, false);
        G.prepare(st.s, "ground-truth", g_counts, g_run_offsets, n_g, memspace, true);
        std::vector<long long> starts((size_t)n_groups + 1, 0);
        for (int k = 0; k < n_groups; ++k) {
            const mrcnn_iou_group& g = groups[k];
            const long long nd = g.d1 - g.d0, ng = g.g1 - g.g0;
            for (long long i = g.d0; i < g.d1 && ng; ++i)        // every RLE of an image has the image's pixels: compare all with the first
                MRCNN_REQUIRE(D.h_tot[(size_t)i] == G.h_tot[(size_t)g.g0], MRCNN_ERR_SHAPE,
                              "rle_iou: group %d: detection %lld sums to %llu pixels, ground truth %lld to %llu", k, i, D.h_tot[(size_t)i],
                              (long long)g.g0, G.h_tot[(size_t)g.g0]);
            for (long long j = g.g0; j < g.g1 && nd; ++j)
                MRCNN_REQUIRE(G.h_tot[(size_t)j] == D.h_tot[(size_t)g.d0], MRCNN_ERR_SHAPE,
                              "rle_iou: group %d: ground truth %lld sums to %llu pixels, detection %lld to %llu", k, j, G.h_tot[(size_t)j],
                              (long long)g.d0, D.h_tot[(size_t)g.d0]);
            starts[(size_t)k + 1] = starts[(size_t)k] + (nd + 3) / 4 * ng;
        }
        const long long n_blocks = starts[(size_t)n_groups];
        MRCNN_REQUIRE(n_blocks < (1LL << 31), MRCNN_ERR_SHAPE, "rle_iou: %lld pairs are too many for one call", pairs);
        if (pairs == 0 || (!inter && !iou)) return;
        const bool dev = memspace == MRCNN_DEVICE;
        DevBuf tg, ts, tc, ti, to;
        upload_groups(tg, ts, groups, n_groups, starts);
        upload_crowd(tc, g_iscrowd, n_g);
        uint32_t* di = inter;
        double* dq = iou;
        if (!dev) {
            if (inter) { ti.alloc((size_t)n_pairs * 4); di = ti.as<uint32_t>(); }
            if (iou) { to.alloc((size_t)n_pairs * 8); dq = to.as<double>(); }
        }
        rle_iou_forward(st.s, D.pre_b.as<uint32_t>(), D.off, D.totals.as<unsigned long long>(), D.areas.as<uint32_t>(), G.pre_b.as<uint32_t>(),
                        G.pre_o.as<uint32_t>(), G.off, G.areas.as<uint32_t>(), tc.as<uint8_t>(), tg.as<IouGroup>(), ts.as<long long>(), n_groups,
                        n_blocks, di, dq);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            if (inter) copy_blocks_to_host(inter, di, groups, n_groups);
            if (iou) copy_blocks_to_host(iou, dq, groups, n_groups);
        }
    });
}

extern "C" int mrcnn_box_iou_xywh(const double* d_boxes, int64_t n_d, const double* g_boxes, int64_t n_g, const uint8_t* g_iscrowd,
                                  const mrcnn_iou_group* groups, int n_groups, int memspace, double* iou, int64_t n_pairs)
{
    return guarded([&] {
        require_gpu();
        const long long pairs = check_iou_groups("box_iou_xywh", groups, n_groups, n_d, n_g, n_pairs);
        MRCNN_REQUIRE((d_boxes || n_d == 0) && (g_boxes || n_g == 0), MRCNN_ERR_INVALID, "box_iou_xywh: null boxes");
        if (pairs == 0 || !iou) return;
        std::vector<long long> starts((size_t)n_groups + 1, 0);
        for (int k = 0; k < n_groups; ++k) starts[(size_t)k + 1] = starts[(size_t)k] + (long long)(groups[k].d1 - groups[k].d0) * (groups[k].g1 - groups[k].g0);
        const bool dev = memspace == MRCNN_DEVICE;
        Stream st;
        DevBuf td, tgb, tg, ts, tc, to;
        const double *db = d_boxes, *gb = g_boxes;
        double* dq = iou;
        if (!dev) {
            td.alloc((size_t)n_d * 32); tgb.alloc((size_t)n_g * 32); to.alloc((size_t)n_pairs * 8);
            HIP_CHECK(hipMemcpy(td.p, d_boxes, (size_t)n_d * 32, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(tgb.p, g_boxes, (size_t)n_g * 32, hipMemcpyHostToDevice));
            db = td.as<double>(); gb = tgb.as<double>(); dq = to.as<double>();
        }
        upload_groups(tg, ts, groups, n_groups, starts);
        upload_crowd(tc, g_iscrowd, n_g);
        box_iou_xywh_forward(st.s, db, gb, tc.as<uint8_t>(), tg.as<IouGroup>(), ts.as<long long>(), n_groups, pairs, dq);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) copy_blocks_to_host(iou, dq, groups, n_groups);
    });
}

extern "C" int mrcnn_coco_match(const double* iou, int64_t n_iou, int memspace, const mrcnn_match_group* groups, int n_groups,
                                const int32_t* dt_idx, const double* dt_area, int64_t n_dt, const int32_t* gt_idx, const double* gt_area,
                                const uint8_t* gt_iscrowd, int64_t n_gt, const double* area_ranges, int n_ranges,
                                const double* iou_thresholds, int n_thresholds, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(n_groups >= 0 && (groups || n_groups == 0) && n_iou >= 0 && n_dt >= 0 && n_gt >= 0 && n_ranges >= 1 && n_thresholds >= 1 &&
                      area_ranges && iou_thresholds, MRCNN_ERR_INVALID, "bad coco_match argument");
        MRCNN_REQUIRE((iou || n_iou == 0) && ((dt_idx && dt_area) || n_dt == 0) && ((gt_idx && gt_area && gt_iscrowd) || n_gt == 0), MRCNN_ERR_INVALID,
                      "coco_match: null table");
        MRCNN_REQUIRE(n_dt < (1LL << 31) && n_gt < (1LL << 31) && (long long)n_groups * n_ranges * n_thresholds < (1LL << 31), MRCNN_ERR_SHAPE,
                      "coco_match: the tables are too large for one call");
        int64_t dt_at = 0, gt_at = 0;
        for (int k = 0; k < n_groups; ++k) {
            const mrcnn_match_group& G = groups[k];
            MRCNN_REQUIRE(G.dt0 == dt_at && G.dt1 >= G.dt0 && G.dt1 <= n_dt && G.gt0 == gt_at && G.gt1 >= G.gt0 && G.gt1 <= n_gt, MRCNN_ERR_SHAPE,
                          "coco_match: group %d has detections [%d, %d) and ground truths [%d, %d): the groups must tile the lists in order (next expected at %lld / %lld)",
                          k, G.dt0, G.dt1, G.gt0, G.gt1, (long long)dt_at, (long long)gt_at);
            dt_at = G.dt1; gt_at = G.gt1;
            MRCNN_REQUIRE(G.iou_stride >= 0 && G.iou_offset >= 0 && G.iou_offset <= n_iou, MRCNN_ERR_SHAPE, "coco_match: group %d: block at %lld with %d columns", k,
                          (long long)G.iou_offset, G.iou_stride);
            int32_t max_row = -1;
            for (int i = G.dt0; i < G.dt1; ++i) {
                MRCNN_REQUIRE(dt_idx[i] >= 0, MRCNN_ERR_SHAPE, "coco_match: dt_idx[%d] = %d", i, dt_idx[i]);
                max_row = dt_idx[i] > max_row ? dt_idx[i] : max_row;
            }
            for (int j = G.gt0; j < G.gt1; ++j)
                MRCNN_REQUIRE(gt_idx[j] >= 0 && gt_idx[j] < G.iou_stride, MRCNN_ERR_SHAPE, "coco_match: gt_idx[%d] = %d is no column of a block of %d", j, gt_idx[j],
                              G.iou_stride);
            if (G.gt1 > G.gt0)
                MRCNN_REQUIRE(G.iou_offset + ((long long)max_row + 1) * G.iou_stride <= n_iou, MRCNN_ERR_SHAPE,
                              "coco_match: group %d reads row %d of its block, beyond the %lld IoU entries", k, max_row, (long long)n_iou);
        }
        MRCNN_REQUIRE(dt_at == n_dt && gt_at == n_gt, MRCNN_ERR_SHAPE, "coco_match: the groups cover %lld of %lld detections and %lld of %lld ground truths",
                      (long long)dt_at, (long long)n_dt, (long long)gt_at, (long long)n_gt);
        if (n_groups == 0) return;
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t AT = (size_t)n_ranges * n_thresholds;
        Stream st;
        DevBuf tq, tg, t1, t2, t3, t4, t5, t6, t7, om, oi, og;
        const double* q = iou;
        if (!dev) { tq.alloc((size_t)n_iou * 8); if (n_iou) HIP_CHECK(hipMemcpy(tq.p, iou, (size_t)n_iou * 8, hipMemcpyHostToDevice)); q = tq.as<double>(); }
        auto up = [](DevBuf& b, const void* src, size_t bytes) { b.alloc(bytes); if (bytes) HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice)); };
        up(tg, groups, (size_t)n_groups * sizeof(mrcnn_match_group));
        up(t1, dt_idx, (size_t)n_dt * 4); up(t2, dt_area, (size_t)n_dt * 8);
        up(t3, gt_idx, (size_t)n_gt * 4); up(t4, gt_area, (size_t)n_gt * 8); up(t5, gt_iscrowd, (size_t)n_gt);
        up(t6, area_ranges, (size_t)n_ranges * 16); up(t7, iou_thresholds, (size_t)n_thresholds * 8);
        int32_t *dm = dt_match, *gm = gt_match;
        uint8_t* di = dt_ignore;
        if (!dev || !dm) { om.alloc(AT * (size_t)n_dt * 4); dm = om.as<int32_t>(); }       // (the kernel writes all three: scratch for the unwanted)
        if (!dev || !di) { oi.alloc(AT * (size_t)n_dt); di = oi.as<uint8_t>(); }
        if (!dev || !gm) { og.alloc(AT * (size_t)n_gt * 4); gm = og.as<int32_t>(); }
        coco_match_forward(st.s, q, tg.as<MatchGroup>(), n_groups, t1.as<int32_t>(), t2.as<double>(), t3.as<int32_t>(), t4.as<double>(), t5.as<uint8_t>(),
                           t6.as<double>(), n_ranges, t7.as<double>(), n_thresholds, dm, di, gm);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            if (dt_match && n_dt) HIP_CHECK(hipMemcpy(dt_match, dm, AT * (size_t)n_dt * 4, hipMemcpyDeviceToHost));
            if (dt_ignore && n_dt) HIP_CHECK(hipMemcpy(dt_ignore, di, AT * (size_t)n_dt, hipMemcpyDeviceToHost));
            if (gt_match && n_gt) HIP_CHECK(hipMemcpy(gt_match, gm, AT * (size_t)n_gt * 4, hipMemcpyDeviceToHost));
        }
    });
}

// COCOeval.accumulate (kernels_coco_acc.hip).  Every argument check comes before the device is touched.
extern "C" int mrcnn_coco_accumulate(const double* scores, const int32_t* ranks, const uint8_t* dt_matched, const uint8_t* dt_ignore, int64_t n_dt,
                                     const int64_t* cat_offsets, int n_cats, const int64_t* npig, int n_ranges, int n_thresholds,
                                     const int32_t* max_dets, int n_max_dets, const double* rec_thrs, int n_rec, int memspace, double* precision,
                                     double* recall)
{
    return guarded([&] {
        MRCNN_REQUIRE(n_dt >= 0 && n_cats >= 0, MRCNN_ERR_INVALID, "coco_accumulate: %lld entries in %d categories", (long long)n_dt, n_cats);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "coco_accumulate: memspace %d", memspace);
        MRCNN_REQUIRE(cat_offsets && max_dets && rec_thrs, MRCNN_ERR_INVALID, "coco_accumulate: null cat_offsets, max_dets or rec_thrs");
        MRCNN_REQUIRE((scores && ranks && dt_matched && dt_ignore) || n_dt == 0, MRCNN_ERR_INVALID, "coco_accumulate: null scores, ranks, dt_matched or dt_ignore");
        MRCNN_REQUIRE((npig && precision && recall) || n_cats == 0, MRCNN_ERR_INVALID, "coco_accumulate: null npig, precision or recall");
        MRCNN_REQUIRE(n_ranges >= 1 && n_thresholds >= 1 && n_max_dets >= 1 && n_rec >= 1, MRCNN_ERR_SHAPE,
                      "coco_accumulate: %d area ranges, %d thresholds, %d max_dets, %d recall thresholds: each must be at least 1", n_ranges, n_thresholds,
                      n_max_dets, n_rec);
        MRCNN_REQUIRE(cat_offsets[0] == 0, MRCNN_ERR_INVALID, "coco_accumulate: cat_offsets[0] = %lld, not 0", (long long)cat_offsets[0]);
        for (int k = 0; k < n_cats; ++k)
            MRCNN_REQUIRE(cat_offsets[k + 1] >= cat_offsets[k], MRCNN_ERR_INVALID, "coco_accumulate: cat_offsets decrease at category %d: [%lld, %lld)", k,
                          (long long)cat_offsets[k], (long long)cat_offsets[k + 1]);
        MRCNN_REQUIRE(cat_offsets[n_cats] == n_dt, MRCNN_ERR_INVALID, "coco_accumulate: cat_offsets end at %lld, the list has %lld entries",
                      (long long)cat_offsets[n_cats], (long long)n_dt);
        for (long long i = 0; i < (long long)n_cats * n_ranges; ++i)
            MRCNN_REQUIRE(npig[i] >= 0, MRCNN_ERR_INVALID, "coco_accumulate: npig of category %lld, area range %lld is %lld", i / n_ranges, i % n_ranges,
                          (long long)npig[i]);
        for (int r = 0; r + 1 < n_rec; ++r)
            MRCNN_REQUIRE(rec_thrs[r + 1] >= rec_thrs[r], MRCNN_ERR_SHAPE, "coco_accumulate: rec_thrs decrease at %d (%g, then %g)", r, rec_thrs[r], rec_thrs[r + 1]);
        MRCNN_REQUIRE(rec_thrs[n_rec - 1] == rec_thrs[n_rec - 1], MRCNN_ERR_SHAPE, "coco_accumulate: rec_thrs[%d] is not a number", n_rec - 1);
        const long long cells = (long long)n_ranges * n_max_dets * n_thresholds;
        MRCNN_REQUIRE(n_dt < (1LL << 31) && cells < (1LL << 31) && (n_cats == 0 || cells < (1LL << 31) / n_cats) &&
                      (long long)n_ranges * n_thresholds < (1LL << 31), MRCNN_ERR_SHAPE, "coco_accumulate: the tables are too large for one call");
        // the chunks of the segments: the grid of the sort
        std::vector<AccChunk> chunks;
        long long longest = 0;
        for (int k = 0; k < n_cats; ++k) {
            const long long len = cat_offsets[k + 1] - cat_offsets[k];
            longest = std::max(longest, len);
            for (long long at = 0; at < len; at += COCO_ACC_CHUNK) chunks.push_back(AccChunk{(long long)cat_offsets[k], (int)len, (int)at});
        }

        require_gpu();
        if (n_cats == 0) return;
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t n = (size_t)n_dt, K = (size_t)n_cats, A = (size_t)n_ranges, T = (size_t)n_thresholds, M = (size_t)n_max_dets, R = (size_t)n_rec;
        Stream st;
        auto up = [](DevBuf& b, const void* src, size_t bytes) { b.alloc(bytes); if (bytes) HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice)); };
        DevBuf t_sc, t_rk, t_dm, t_di, t_ch, t_off, t_np, t_md, t_th, t_ka, t_kb, t_pa, t_pb, t_code, t_srank, t_pr, t_rc;
        const double* d_sc = scores;
        const int32_t* d_rk = ranks;
        const uint8_t *d_dm = dt_matched, *d_di = dt_ignore;
        double *d_pr = precision, *d_rc = recall;
        if (!dev) {
            up(t_sc, scores, n * 8); up(t_rk, ranks, n * 4); up(t_dm, dt_matched, A * T * n); up(t_di, dt_ignore, A * T * n);
            t_pr.alloc(T * R * K * A * M * 8); t_rc.alloc(T * K * A * M * 8);
            d_sc = t_sc.as<double>(); d_rk = t_rk.as<int32_t>(); d_dm = t_dm.as<uint8_t>(); d_di = t_di.as<uint8_t>();
            d_pr = t_pr.as<double>(); d_rc = t_rc.as<double>();
        }
        up(t_ch, chunks.data(), chunks.size() * sizeof(AccChunk));
        up(t_off, cat_offsets, (K + 1) * 8); up(t_np, npig, K * A * 8); up(t_md, max_dets, M * 4); up(t_th, rec_thrs, R * 8);
        t_ka.alloc(n * 8); t_kb.alloc(n * 8); t_pa.alloc(n * 4); t_pb.alloc(n * 4); t_code.alloc(A * T * n); t_srank.alloc(n * 4);
        const uint32_t* perm = coco_acc_sort_forward(st.s, d_sc, t_ch.as<AccChunk>(), (long)chunks.size(), longest, t_ka.as<unsigned long long>(),
                                                     t_pa.as<uint32_t>(), t_kb.as<unsigned long long>(), t_pb.as<uint32_t>());
        coco_acc_permute_forward(st.s, perm, d_rk, d_dm, d_di, (long long)n_dt, (int)(A * T), t_code.as<uint8_t>(), t_srank.as<int32_t>());
        coco_acc_scan_forward(st.s, t_code.as<uint8_t>(), t_srank.as<int32_t>(), t_off.as<long long>(), t_np.as<long long>(), t_md.as<int32_t>(),
                              t_th.as<double>(), (long long)n_dt, n_cats, n_ranges, n_max_dets, n_thresholds, n_rec, d_pr, d_rc);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(precision, d_pr, T * R * K * A * M * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(recall, d_rc, T * K * A * M * 8, hipMemcpyDeviceToHost));
        }
    });
}

// COCO's rleFrPoly restated (host arithmetic).  One polygon -> the sorted positions where the column-major pixel stream toggles.
namespace {
void polygon_toggles(const double* xy, int64_t k, long h, long w, std::vector<uint32_t>& out)
{
    out.clear();
    if (k <= 0) return;
    const double scale = 5.0;
    std::vector<long> x((size_t)k + 1), y((size_t)k + 1);
    for (int64_t j = 0; j < k; ++j) { x[(size_t)j] = (long)(int)(scale * xy[2 * j] + .5); y[(size_t)j] = (long)(int)(scale * xy[2 * j + 1] + .5); }
    x[(size_t)k] = x[0]; y[(size_t)k] = y[0];
    std::vector<long> u, v;                                  // every fine-grid point along the outline, edge after edge
    for (int64_t j = 0; j < k; ++j) {
        long xs = x[(size_t)j], xe = x[(size_t)j + 1], ys = y[(size_t)j], ye = y[(size_t)j + 1];
        const long dx = labs(xe - xs), dy = labs(ys - ye);
        const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
        if (flip) { std::swap(xs, xe); std::swap(ys, ye); }
        const long span = dx >= dy ? dx : dy;
        const double s = span == 0 ? 0.0 : (dx >= dy ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy);
        for (long d = 0; d <= span; ++d) {
            const long t = flip ? span - d : d;
            if (dx >= dy) { u.push_back(t + xs); v.push_back((long)(int)(ys + s * t + .5)); }
            else { v.push_back(t + ys); u.push_back((long)(int)(xs + s * t + .5)); }
        }
    }
    // where the outline steps from one fine column to the next AND that step crosses a pixel-column centre: one run boundary
    for (size_t j = 1; j < u.size(); ++j) {
        if (u[j] == u[j - 1]) continue;
        double xd = (double)(u[j] < u[j - 1] ? u[j] : u[j] - 1);
        xd = (xd + .5) / scale - .5;
        if (floor(xd) != xd || xd < 0 || xd > (double)(w - 1)) continue;
        double yd = (double)(v[j] < v[j - 1] ? v[j] : v[j - 1]);
        yd = (yd + .5) / scale - .5;
        if (yd < 0) yd = 0; else if (yd > (double)h) yd = (double)h;
        yd = ceil(yd);
        out.push_back((uint32_t)((long)xd * h + (long)yd));
    }
    std::sort(out.begin(), out.end());
}

// toggle positions -> the set intervals [s, e) (equal positions cancel in pairs, like the zero-length runs rleFrPoly drops)
void toggles_to_intervals(const std::vector<uint32_t>& tg, uint32_t total, std::vector<std::pair<uint32_t, uint32_t>>& iv)
{
    bool on = false;
    uint32_t start = 0;
    for (size_t i = 0; i < tg.size(); ++i) {
        if (!on) { start = tg[i]; on = true; }
        else { if (tg[i] > start) iv.emplace_back(start, tg[i]); on = false; }
    }
    if (on && total > start) iv.emplace_back(start, total);
}
}  // namespace

extern "C" int mrcnn_rle_from_polygons(const double* xy, const int64_t* poly_offsets, int n_polys, int h, int w, uint32_t* counts,
                                       int64_t capacity, int64_t* n)
{
    return guarded([&] {
        MRCNN_REQUIRE(n && n_polys >= 0 && (poly_offsets || n_polys == 0) && capacity >= 0 && (counts || capacity == 0), MRCNN_ERR_INVALID,
                      "bad rle_from_polygons argument");
        MRCNN_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, MRCNN_ERR_SHAPE, "rle_from_polygons: the plane is %dx%d: height and width must lie in 1..32767", h, w);
        const uint32_t total = (uint32_t)h * (uint32_t)w;
        std::vector<std::pair<uint32_t, uint32_t>> iv;
        std::vector<uint32_t> tg;
        for (int p = 0; p < n_polys; ++p) {
            const int64_t k = poly_offsets[p + 1] - poly_offsets[p];
            MRCNN_REQUIRE(poly_offsets[p] >= 0 && k >= 0 && (xy || k == 0), MRCNN_ERR_SHAPE, "rle_from_polygons: polygon %d has the point range [%lld, %lld)", p,
                          (long long)poly_offsets[p], (long long)poly_offsets[p + 1]);
            for (int64_t i = 2 * poly_offsets[p]; i < 2 * poly_offsets[p + 1]; ++i)
                MRCNN_REQUIRE(fabs(xy[i]) < 1e6, MRCNN_ERR_INVALID, "rle_from_polygons: coordinate %lld of polygon %d is not a finite pixel position", (long long)(i - 2 * poly_offsets[p]), p);
            polygon_toggles(xy + 2 * poly_offsets[p], k, h, w, tg);
            toggles_to_intervals(tg, total, iv);
        }
        // the union of the polygons' intervals, then the run lengths
        std::sort(iv.begin(), iv.end());
        std::vector<uint32_t> runs;
        uint32_t at = 0;                      // end of what has been emitted: the stream is zero from here on until the next interval
        size_t i = 0;
        while (i < iv.size()) {
            uint32_t s = iv[i].first, e = iv[i].second;
            for (++i; i < iv.size() && iv[i].first <= e; ++i) e = iv[i].second > e ? iv[i].second : e;
            runs.push_back(s - at); runs.push_back(e - s);
            at = e;
        }
        if (at < total || runs.empty()) runs.push_back(total - at);
        *n = (int64_t)runs.size();
        MRCNN_REQUIRE(*n <= capacity || !counts, MRCNN_ERR_SHAPE, "rle_from_polygons: the mask has %lld runs, counts holds %lld", (long long)*n, (long long)capacity);
        if (counts) memcpy(counts, runs.data(), runs.size() * sizeof(uint32_t));
    });
}

// The same for a whole annotation file at once, on the device (kernels_coco.hip, poly_device.h).  Every argument check comes before
// the device is touched.
extern "C" int mrcnn_rle_from_polygons_batch(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, int64_t n_anns,
                                             const int32_t* heights, const int32_t* widths, int memspace, uint32_t* counts, int64_t capacity,
                                             int64_t* run_offsets, uint32_t* areas, int32_t* bboxes_xywh)
{
    return guarded([&] {
        MRCNN_REQUIRE(n_anns >= 0 && ann_offsets && run_offsets && ((heights && widths) || n_anns == 0), MRCNN_ERR_INVALID,
                      "rle_from_polygons_batch: null table or negative number of annotations");
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "rle_from_polygons_batch: memspace %d", memspace);
        MRCNN_REQUIRE(capacity >= 0 && (counts || capacity == 0), MRCNN_ERR_INVALID, "rle_from_polygons_batch: null counts with capacity %lld",
                      (long long)capacity);
        MRCNN_REQUIRE(n_anns < (1LL << 31), MRCNN_ERR_SHAPE, "rle_from_polygons_batch: %lld annotations are too many for one call", (long long)n_anns);
        MRCNN_REQUIRE(ann_offsets[0] >= 0, MRCNN_ERR_INVALID, "rle_from_polygons_batch: ann_offsets[0] = %lld is negative", (long long)ann_offsets[0]);
        for (int64_t k = 0; k < n_anns; ++k) {
            MRCNN_REQUIRE(ann_offsets[k + 1] >= ann_offsets[k], MRCNN_ERR_INVALID, "rle_from_polygons_batch: annotation %lld has the polygon range [%lld, %lld)",
                          (long long)k, (long long)ann_offsets[k], (long long)ann_offsets[k + 1]);
            MRCNN_REQUIRE(heights[k] >= 1 && heights[k] <= 32767 && widths[k] >= 1 && widths[k] <= 32767, MRCNN_ERR_SHAPE,
                          "rle_from_polygons_batch: the plane of annotation %lld is %dx%d: height and width must lie in 1..32767", (long long)k, heights[k],
                          widths[k]);
        }
        const int64_t p0 = ann_offsets[0], p1 = ann_offsets[n_anns];
        MRCNN_REQUIRE(poly_offsets || p1 == p0, MRCNN_ERR_INVALID, "rle_from_polygons_batch: null poly_offsets");
        MRCNN_REQUIRE(p1 - p0 < (1LL << 31), MRCNN_ERR_SHAPE, "rle_from_polygons_batch: %lld polygons are too many for one call", (long long)(p1 - p0));
        const int64_t pt_base = p1 > p0 ? poly_offsets[p0] : 0;
        MRCNN_REQUIRE(pt_base >= 0, MRCNN_ERR_INVALID, "rle_from_polygons_batch: poly_offsets[%lld] = %lld is negative", (long long)p0, (long long)pt_base);
        std::vector<PolyRec> polys((size_t)(p1 - p0));
        std::vector<PolyAnn> anns((size_t)n_anns);
        for (int64_t k = 0; k < n_anns; ++k) {
            for (int64_t p = ann_offsets[k]; p < ann_offsets[k + 1]; ++p) {
                const long long q = (long long)(p - ann_offsets[k]);
                const int64_t a = poly_offsets[p], b = poly_offsets[p + 1];
                MRCNN_REQUIRE(b >= a && b - pt_base < (1LL << 31), b >= a ? MRCNN_ERR_SHAPE : MRCNN_ERR_INVALID,
                              "rle_from_polygons_batch: polygon %lld of annotation %lld has the point range [%lld, %lld)", q, (long long)k, (long long)a, (long long)b);
                MRCNN_REQUIRE(xy || b == a, MRCNN_ERR_INVALID, "rle_from_polygons_batch: null xy");
                for (int64_t i = 2 * a; i < 2 * b; ++i)
                    MRCNN_REQUIRE(fabs(xy[i]) < 1e6, MRCNN_ERR_INVALID,
                                  "rle_from_polygons_batch: coordinate %lld of polygon %lld of annotation %lld is not a finite pixel position", (long long)(i - 2 * a), q,
                                  (long long)k);
                polys[(size_t)(p - p0)] = PolyRec{(long long)(a - pt_base), (int)(b - a), (int)k};
            }
            const long long f = ann_offsets[k] < p1 ? poly_offsets[ann_offsets[k]] - pt_base : (p1 > p0 ? poly_offsets[p1] - pt_base : 0);
            anns[(size_t)k] = PolyAnn{f, 0, (int)(ann_offsets[k] - p0), heights[k], widths[k], 0};
        }
        const long n_pts = p1 > p0 ? (long)(poly_offsets[p1] - pt_base) : 0;
        for (int64_t k = 0; k < n_anns; ++k) anns[(size_t)k].pt1 = k + 1 < n_anns ? anns[(size_t)k + 1].pt0 : n_pts;
        std::vector<int32_t> pt_poly((size_t)n_pts);
        for (size_t p = 0; p < polys.size(); ++p)
            for (int j = 0; j < polys[p].npts; ++j) pt_poly[(size_t)polys[p].pt0 + (size_t)j] = (int32_t)p;

        require_gpu();
        const bool dev = memspace == MRCNN_DEVICE;
        const size_t n = (size_t)n_anns;
        Stream st;
        auto up = [](DevBuf& b, const void* src, size_t bytes) { b.alloc(bytes ? bytes : 16); if (bytes) HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice)); };
        DevBuf t_xy, t_pp, t_pr, t_an, t_ec, t_es, t_to, t_bnd, t_nb, t_nr, t_ro, t_ar, t_bb, t_big, t_keys, t_cov, t_c;
        up(t_xy, xy ? xy + 2 * pt_base : nullptr, (size_t)n_pts * 16);
        up(t_pp, pt_poly.data(), (size_t)n_pts * 4);
        up(t_pr, polys.data(), polys.size() * sizeof(PolyRec));
        up(t_an, anns.data(), n * sizeof(PolyAnn));
        t_ec.alloc((size_t)n_pts * 4 + 16); t_es.alloc(((size_t)n_pts + 1) * 8); t_to.alloc((n + 1) * 8);
        poly_count_forward(st.s, t_xy.as<double>(), t_pp.as<int32_t>(), t_pr.as<PolyRec>(), t_an.as<PolyAnn>(), n_pts, (long)n_anns, t_ec.as<uint32_t>(),
                           t_es.as<long long>(), t_to.as<long long>());
        std::vector<long long> tog((size_t)n + 1, 0);
        HIP_CHECK(hipMemcpyAsync(tog.data(), t_to.p, (n + 1) * 8, hipMemcpyDeviceToHost, st.s));
        HIP_CHECK(hipStreamSynchronize(st.s));
        // the annotations whose toggles do not fit LDS are sorted in global memory, each in a power-of-two slice of one scratch
        std::vector<PolyBig> big;
        long long scratch = 0;
        for (size_t k = 0; k < n; ++k) {
            const long long m = tog[k + 1] - tog[k];
            if (m <= POLY_LDS_TOGGLES) continue;
            long long padded = 1;
            while (padded < m) padded <<= 1;
            big.push_back(PolyBig{(long long)k, scratch, padded});
            scratch += padded;
        }
        MRCNN_REQUIRE(big.size() < (1u << 31), MRCNN_ERR_SHAPE, "rle_from_polygons_batch: too many large annotations for one call");
        long long* ro = reinterpret_cast<long long*>(run_offsets);
        uint32_t* ar = areas;
        int32_t* bb = bboxes_xywh;
        if (!dev) {
            t_ro.alloc((n + 1) * 8); ro = t_ro.as<long long>();
            if (areas) { t_ar.alloc(n * 4 + 16); ar = t_ar.as<uint32_t>(); }
            if (bboxes_xywh) { t_bb.alloc(n * 16 + 16); bb = t_bb.as<int32_t>(); }
        }
        t_bnd.alloc((size_t)tog[n] * 4 + 16); t_nb.alloc(n * 4 + 16); t_nr.alloc(n * 4 + 16);
        poly_encode_lds_forward(st.s, t_xy.as<double>(), t_pp.as<int32_t>(), t_pr.as<PolyRec>(), t_an.as<PolyAnn>(), (long)n_anns, t_es.as<long long>(),
                                t_bnd.as<uint32_t>(), t_nb.as<uint32_t>(), t_nr.as<uint32_t>(), ar, bb);
        if (!big.empty()) {
            up(t_big, big.data(), big.size() * sizeof(PolyBig));
            t_keys.alloc((size_t)scratch * 8); t_cov.alloc((size_t)scratch * 4);
            poly_encode_big_forward(st.s, t_xy.as<double>(), t_pp.as<int32_t>(), t_pr.as<PolyRec>(), t_an.as<PolyAnn>(), t_es.as<long long>(),
                                    t_big.as<PolyBig>(), big.data(), (int)big.size(), t_keys.as<unsigned long long>(), t_cov.as<int32_t>(),
                                    t_bnd.as<uint32_t>(), t_nb.as<uint32_t>(), t_nr.as<uint32_t>(), ar, bb);
        }
        poly_offsets_forward(st.s, t_nr.as<uint32_t>(), (long)n_anns, ro);
        long long need = 0;
        HIP_CHECK(hipMemcpyAsync(&need, ro + n, sizeof(need), hipMemcpyDeviceToHost, st.s));
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) {
            HIP_CHECK(hipMemcpy(run_offsets, t_ro.p, (n + 1) * 8, hipMemcpyDeviceToHost));
            if (areas && n) HIP_CHECK(hipMemcpy(areas, t_ar.p, n * 4, hipMemcpyDeviceToHost));
            if (bboxes_xywh && n) HIP_CHECK(hipMemcpy(bboxes_xywh, t_bb.p, n * 16, hipMemcpyDeviceToHost));
        }
        // everything but the runs is written by now; the runs only when all of them fit
        MRCNN_REQUIRE(need <= (long long)capacity, MRCNN_ERR_SHAPE,
                      "rle_from_polygons_batch: the annotations encode to %lld runs, counts holds %lld: call again with capacity >= %lld", need,
                      (long long)capacity, need);
        if (n == 0) return;
        uint32_t* c = counts;
        if (!dev) { t_c.alloc((size_t)need * 4); c = t_c.as<uint32_t>(); }
        poly_write_forward(st.s, t_an.as<PolyAnn>(), (long)n_anns, t_to.as<long long>(), t_bnd.as<uint32_t>(), t_nb.as<uint32_t>(), ro, c);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (!dev) HIP_CHECK(hipMemcpy(counts, t_c.p, (size_t)need * 4, hipMemcpyDeviceToHost));
    });
}
