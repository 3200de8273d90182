// rle_morph_host.cpp — see rle_morph_host.h.  The rule of include/maskrcnn_hip.h as it reads, sequential and plain on purpose: this file
// is what the kernels of kernels_rle_morph.hip are compared with.
#include "rle_morph_host.h"

#include <algorithm>

#include "morph_rule.h"

namespace mrcnn {
namespace rle_morph {

int check_arguments(const Set& s, const uint32_t* out_counts, int64_t capacity, const int64_t* out_run_offsets, const char* who, std::string* err)
{
    int st = rle_set::check_flat_pointers(s, who, err);
    if (st != MRCNN_OK) return st;
    if (!out_run_offsets || (!s.radii && s.n > 0)) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (capacity < 0 || (!out_counts && capacity != 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null out_counts with capacity %lld", who, (long long)capacity);
    if (s.op != MRCNN_MORPH_ERODE && s.op != MRCNN_MORPH_DILATE && s.op != MRCNN_MORPH_BOUNDARY)
        return bad(err, MRCNN_ERR_SHAPE, "%s: unknown op %d", who, s.op);
    // The lowest RLE that fails is named, its sides before its radius: so the sides are judged as far as the first bad radius, k.
    const bool countable = s.n < (1LL << 31);                    // (too many RLEs are refused before any is read)
    int64_t k = 0;
    while (countable && k < s.n && s.radii[k] >= 0 && s.radii[k] <= MRCNN_MORPH_MAX_RADIUS) ++k;
    rle_set::Flat judged = s;
    if (countable && k < s.n) judged.n = k + 1;
    st = rle_set::check_flat_sides(judged, who, err);
    if (st != MRCNN_OK || k == s.n) return st;
    return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld has radius %d: a radius must lie in 0..MRCNN_MORPH_MAX_RADIUS = %d", who, (long long)k, s.radii[k],
               MRCNN_MORPH_MAX_RADIUS);
}

namespace {

// One half of the square on the `lines` lines of `len` pixels of a plane (pixel i of line l at l*line_stride + i*pixel_stride): the
// window [i - r, i + r], cut at the line's ends, holds S[hi] - S[lo] set pixels by the running count S.  Erosion wants all 2r + 1 —
// a window cut by an end is short of some: outside is 0 — and dilation wants one.
void half(const uint8_t* in, uint8_t* out, int lines, int len, size_t line_stride, size_t pixel_stride, int r, bool grows, std::vector<int32_t>& S)
{
    S.resize((size_t)len + 1);
    for (int l = 0; l < lines; ++l) {
        const uint8_t* src = in + l * line_stride;
        uint8_t* dst = out + l * line_stride;
        S[0] = 0;
        for (int i = 0; i < len; ++i) S[(size_t)i + 1] = S[(size_t)i] + src[i * pixel_stride];
        for (int i = 0; i < len; ++i) {
            const int count = S[(size_t)std::min(len, i + r + 1)] - S[(size_t)std::max(0, i - r)];
            dst[i * pixel_stride] = grows ? count > 0 : count == 2 * r + 1;
        }
    }
}

struct Encoded { std::vector<uint32_t> runs; uint32_t area; int32_t box[4]; };

}  // namespace

int morph_host(const Set& s, uint32_t* out_counts, int64_t capacity, int64_t* out_run_offsets, uint32_t* areas, int32_t* bboxes_xywh, std::string* err)
{
    const char* who = "rle_morph_host";
    int st = check_arguments(s, out_counts, capacity, out_run_offsets, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    std::vector<Encoded> done((size_t)s.n);
    std::vector<uint8_t> P, V, R;                                // column-major planes: pixel (y, x) at x*h + y
    std::vector<int32_t> S;
    long long need = 0;
    for (int64_t k = 0; k < s.n; ++k) {
        const int h = s.heights[k], w = s.widths[k], r = s.radii[k];
        const size_t hw = (size_t)h * w;
        const bool grows = morph_grows(s.op);
        P.assign(hw, 0); V.resize(hw); R.resize(hw);
        size_t p = 0;
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
            const uint32_t c = s.counts[j];
            if ((j - s.run_offsets[k]) & 1) std::fill(P.begin() + (ptrdiff_t)p, P.begin() + (ptrdiff_t)(p + c), (uint8_t)1);
            p += c;
        }
        half(P.data(), V.data(), w, h, (size_t)h, 1, r, grows, S);               // along the columns
        half(V.data(), R.data(), h, w, 1, (size_t)h, r, grows, S);               // along the rows
        if (s.op == MRCNN_MORPH_BOUNDARY)
            for (size_t i = 0; i < hw; ++i) R[i] = P[i] & (uint8_t)!R[i];

        Encoded& e = done[(size_t)k];
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
    for (int64_t k = 0; k < s.n; ++k) {
        out_run_offsets[k + 1] = out_run_offsets[k] + (int64_t)done[(size_t)k].runs.size();
        if (areas) areas[k] = done[(size_t)k].area;
        if (bboxes_xywh) std::copy(done[(size_t)k].box, done[(size_t)k].box + 4, bboxes_xywh + 4 * k);
    }
    if (need > (long long)capacity) return rle_set::bad_runs_capacity(need, (long long)capacity, who, err);
    for (int64_t k = 0; k < s.n; ++k) std::copy(done[(size_t)k].runs.begin(), done[(size_t)k].runs.end(), out_counts + out_run_offsets[k]);
    return MRCNN_OK;
}

}  // namespace rle_morph
}  // namespace mrcnn
