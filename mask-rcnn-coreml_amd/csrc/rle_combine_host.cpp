// rle_combine_host.cpp — see rle_combine_host.h.  The rule of include/maskrcnn_hip.h as it reads, sequential and plain on purpose: this
// file is what the kernel of kernels_rle_combine.hip is compared with.
#include "rle_combine_host.h"

#include <algorithm>

#include "combine_rule.h"

namespace mrcnn {
namespace rle_combine {

int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err)
{
    if (s.n >= 0 && s.n_groups < 0) return bad(err, MRCNN_ERR_SHAPE, "%s: n_groups %lld is negative", who, (long long)s.n_groups);      // (n is judged first)
    int st = rle_set::check_flat_pointers(s, who, err);
    if (st != MRCNN_OK) return st;
    if (!out_run_offsets || !s.group_offsets) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (capacity < 0 || (!out_counts && capacity != 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null out_counts with capacity %lld", who, (long long)capacity);
    if (!combine_known(s.op)) return bad(err, MRCNN_ERR_SHAPE, "%s: unknown op %d", who, s.op);
    if (s.n >= (1LL << 31) || s.n_groups >= (1LL << 31))
        return bad(err, MRCNN_ERR_SHAPE, "%s: %lld RLEs in %lld groups are too many", who, (long long)s.n, (long long)s.n_groups);
    st = rle_set::check_flat_sides(s, who, err);
    if (st != MRCNN_OK) return st;
    if (s.group_offsets[0] != 0) return bad(err, MRCNN_ERR_SHAPE, "%s: group_offsets[0] is %lld, not 0", who, (long long)s.group_offsets[0]);
    for (int64_t g = 0; g < s.n_groups; ++g) {
        if (s.group_offsets[g + 1] < s.group_offsets[g])
            return bad(err, MRCNN_ERR_SHAPE, "%s: group_offsets decrease at group %lld: %lld after %lld", who, (long long)g, (long long)s.group_offsets[g + 1],
                       (long long)s.group_offsets[g]);
        if (s.group_offsets[g + 1] == s.group_offsets[g]) return bad(err, MRCNN_ERR_SHAPE, "%s: group %lld is empty: a group needs a member", who, (long long)g);
    }
    if (s.n_groups > 0 && !s.members) return bad(err, MRCNN_ERR_INVALID, "%s: null members", who);
    for (int64_t g = 0; g < s.n_groups; ++g) {
        const int64_t first = s.members[s.group_offsets[g]];
        for (int64_t j = s.group_offsets[g]; j < s.group_offsets[g + 1]; ++j) {
            const int64_t m = s.members[j], at = j - s.group_offsets[g];
            if (m < 0 || m >= s.n)
                return bad(err, MRCNN_ERR_SHAPE, "%s: group %lld member %lld is RLE %lld: outside 0..%lld", who, (long long)g, (long long)at, (long long)m,
                           (long long)s.n - 1);
            if (s.heights[m] != s.heights[first] || s.widths[m] != s.widths[first])
                return bad(err, MRCNN_ERR_SHAPE, "%s: group %lld member %lld (RLE %lld) is %dx%d, the group's first member (RLE %lld) %dx%d", who, (long long)g,
                           (long long)at, (long long)m, s.heights[m], s.widths[m], (long long)first, s.heights[first], s.widths[first]);
        }
    }
    return MRCNN_OK;
}

namespace {
struct Encoded { std::vector<uint32_t> runs; uint32_t area; int32_t box[4]; };
}  // namespace

int combine_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err)
{
    const char* who = "rle_combine_host";
    int st = check_arguments(s, out_counts, capacity, out_run_offsets, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    std::vector<Encoded> done((size_t)s.n_groups);
    std::vector<uint8_t> R, M;                                   // column-major planes: pixel (y, x) at x*h + y
    auto decode = [&](int64_t k, std::vector<uint8_t>& P, size_t hw) {
        P.assign(hw, 0);
        size_t p = 0;
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
            const uint32_t c = s.counts[j];
            if ((j - s.run_offsets[k]) & 1) std::fill(P.begin() + (ptrdiff_t)p, P.begin() + (ptrdiff_t)(p + c), (uint8_t)1);
            p += c;
        }
    };
    long long need = 0;
    for (int64_t g = 0; g < s.n_groups; ++g) {
        const int64_t first = s.members[s.group_offsets[g]];
        const int h = s.heights[first], w = s.widths[first];
        const size_t hw = (size_t)h * w;
        decode(first, R, hw);
        for (int64_t j = s.group_offsets[g] + 1; j < s.group_offsets[g + 1]; ++j) {
            decode(s.members[j], M, hw);
            for (size_t i = 0; i < hw; ++i) R[i] = combine_fold<uint8_t>(s.op, R[i], M[i]) & 1;
        }

        Encoded& e = done[(size_t)g];
        e.area = 0;
        int xmin = w, ymin = h, xmax = -1, ymax = -1;
        uint8_t cur = 0;
        size_t start = 0;
        for (size_t i = 0; i < hw; ++i) {
            if (R[i] != cur) { e.runs.push_back((uint32_t)(i - start)); start = i; cur = R[i]; }
            if (!R[i]) continue;
            const int x = (int)(i / (size_t)h), y = (int)(i % (size_t)h);
            ++e.area;
            xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
        }
        e.runs.push_back((uint32_t)(hw - start));
        const bool any = e.area > 0;
        e.box[0] = any ? xmin : 0; e.box[1] = any ? ymin : 0; e.box[2] = any ? xmax - xmin + 1 : 0; e.box[3] = any ? ymax - ymin + 1 : 0;
        need += (long long)e.runs.size();
    }

    // everything but the runs is written whatever the capacity; the runs only when all of them fit
    out_run_offsets[0] = 0;
    for (int64_t g = 0; g < s.n_groups; ++g) {
        out_run_offsets[g + 1] = out_run_offsets[g] + (int64_t)done[(size_t)g].runs.size();
        if (areas) areas[g] = done[(size_t)g].area;
        if (bboxes_xywh) std::copy(done[(size_t)g].box, done[(size_t)g].box + 4, bboxes_xywh + 4 * g);
    }
    if (need > (long long)capacity) return rle_set::bad_runs_capacity(need, (long long)capacity, who, err);
    for (int64_t g = 0; g < s.n_groups; ++g) std::copy(done[(size_t)g].runs.begin(), done[(size_t)g].runs.end(), out_counts + out_run_offsets[g]);
    return MRCNN_OK;
}

}  // namespace rle_combine
}  // namespace mrcnn
