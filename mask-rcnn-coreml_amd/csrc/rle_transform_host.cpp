// rle_transform_host.cpp — see rle_transform_host.h.  The rule of include/maskrcnn_hip.h as it reads, sequential and plain on purpose:
// this file is what the kernel of kernels_rle_transform.hip is compared with.
#include "rle_transform_host.h"

#include <algorithm>

#include "transform_rule.h"

namespace mrcnn {
namespace rle_transform {

int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err)
{
    int st = rle_set::check_flat_pointers(s, who, err);
    if (st != MRCNN_OK) return st;
    if (!out_run_offsets || ((!s.out_heights || !s.out_widths || !s.xf) && s.n > 0)) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (capacity < 0 || (!out_counts && capacity != 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null out_counts with capacity %lld", who, (long long)capacity);
    st = rle_set::check_flat_sides(s, who, err);
    if (st != MRCNN_OK) return st;
    for (int64_t k = 0; k < s.n; ++k) {
        if (s.out_heights[k] < 1 || s.out_heights[k] > 32767 || s.out_widths[k] < 1 || s.out_widths[k] > 32767)
            return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld goes to a %dx%d plane: height and width must lie in 1..32767", who, (long long)k, s.out_heights[k],
                       s.out_widths[k]);
        const int64_t* r = s.xf + 8 * k;
        if (r[0] & ~(int64_t)MRCNN_XF_TRANSPOSE)
            return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld has flags %lld: only MRCNN_XF_TRANSPOSE = %d is known", who, (long long)k, (long long)r[0], MRCNN_XF_TRANSPOSE);
        if (!xf_axis_known(r[1], r[2], r[3]))
            return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld has ax, bx, dx = %lld, %lld, %lld: 1 <= |ax|, dx <= 2^31-1 and |bx| <= 2^46 expected", who, (long long)k,
                       (long long)r[1], (long long)r[2], (long long)r[3]);
        if (!xf_axis_known(r[4], r[5], r[6]))
            return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld has ay, by, dy = %lld, %lld, %lld: 1 <= |ay|, dy <= 2^31-1 and |by| <= 2^46 expected", who, (long long)k,
                       (long long)r[4], (long long)r[5], (long long)r[6]);
        if (r[7] != 0) return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld has %lld in word 7 of its record: it must be 0", who, (long long)k, (long long)r[7]);
    }
    return MRCNN_OK;
}

namespace {
struct Encoded { std::vector<uint32_t> runs; uint32_t area; int32_t box[4]; };
}  // namespace

int transform_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err)
{
    const char* who = "rle_transform_host";
    int st = check_arguments(s, out_counts, capacity, out_run_offsets, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    std::vector<Encoded> done((size_t)s.n);
    std::vector<uint8_t> P, R;                                   // column-major planes: pixel (y, x) at x*h + y
    long long need = 0;
    for (int64_t k = 0; k < s.n; ++k) {
        const int h = s.heights[k], w = s.widths[k], oh = s.out_heights[k], ow = s.out_widths[k];
        const XfMap m = xf_map(s.xf + 8 * k);
        P.assign((size_t)h * w, 0);
        size_t p = 0;
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
            const uint32_t c = s.counts[j];
            if ((j - s.run_offsets[k]) & 1) std::fill(P.begin() + (ptrdiff_t)p, P.begin() + (ptrdiff_t)(p + c), (uint8_t)1);
            p += c;
        }
        const size_t hw = (size_t)oh * ow;
        R.assign(hw, 0);
        for (int X = 0; X < ow; ++X)
            for (int Y = 0; Y < oh; ++Y) {
                const long long u = xf_source(m.x, X), v = xf_source(m.y, Y);
                const long long sx = m.transpose ? v : u, sy = m.transpose ? u : v;
                if (sx >= 0 && sx < w && sy >= 0 && sy < h) R[(size_t)X * oh + Y] = P[(size_t)sx * h + (size_t)sy];
            }

        Encoded& e = done[(size_t)k];
        e.area = 0;
        int xmin = ow, ymin = oh, xmax = -1, ymax = -1;
        uint8_t cur = 0;
        size_t start = 0;
        for (size_t i = 0; i < hw; ++i) {
            if (R[i] != cur) { e.runs.push_back((uint32_t)(i - start)); start = i; cur = R[i]; }
            if (!R[i]) continue;
            const int x = (int)(i / (size_t)oh), y = (int)(i % (size_t)oh);
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
    for (int64_t k = 0; k < s.n; ++k) {
        out_run_offsets[k + 1] = out_run_offsets[k] + (int64_t)done[(size_t)k].runs.size();
        if (areas) areas[k] = done[(size_t)k].area;
        if (bboxes_xywh) std::copy(done[(size_t)k].box, done[(size_t)k].box + 4, bboxes_xywh + 4 * k);
    }
    if (need > (long long)capacity) return rle_set::bad_runs_capacity(need, (long long)capacity, who, err);
    for (int64_t k = 0; k < s.n; ++k) std::copy(done[(size_t)k].runs.begin(), done[(size_t)k].runs.end(), out_counts + out_run_offsets[k]);
    return MRCNN_OK;
}

}  // namespace rle_transform
}  // namespace mrcnn
