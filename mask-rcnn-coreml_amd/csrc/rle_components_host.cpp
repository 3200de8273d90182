// rle_components_host.cpp — see rle_components_host.h.  The rule of include/maskrcnn_hip.h as it reads, sequential and plain on
// purpose: this file is what the kernels of kernels_rle_components.hip are compared with.
#include "rle_components_host.h"

#include <algorithm>

#include "components_rule.h"

namespace mrcnn {
namespace rle_components {

int check_set(const Set& s, const char* who, std::string* err)
{
    const int st = rle_set::check_flat_pointers(s, who, err);
    if (st != MRCNN_OK) return st;
    if (s.connectivity != 4 && s.connectivity != 8) return bad(err, MRCNN_ERR_SHAPE, "%s: connectivity %d is neither 4 nor 8", who, s.connectivity);
    if (s.of != MRCNN_COMPONENTS_OF_ONES && s.of != MRCNN_COMPONENTS_OF_ZEROS) return bad(err, MRCNN_ERR_SHAPE, "%s: unknown of %d", who, s.of);
    return rle_set::check_flat_sides(s, who, err);
}

int check_measures(const Set& s, const Measures& m, const char* who, std::string* err)
{
    const int st = check_set(s, who, err);
    if (st != MRCNN_OK) return st;
    if (!m.comp_offsets) return bad(err, MRCNN_ERR_INVALID, "%s: null comp_offsets", who);
    if (m.comp_capacity < 0 || ((!m.comp_areas || !m.comp_bboxes_xywh || !m.comp_flags) && m.comp_capacity != 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null component array with comp_capacity %lld", who, (long long)m.comp_capacity);
    return MRCNN_OK;
}

int check_select(const Set& s, const Select& q, const char* who, std::string* err)
{
    const int st = check_set(s, who, err);
    if (st != MRCNN_OK) return st;
    if (q.mode != MRCNN_COMPONENTS_MERGE && q.mode != MRCNN_COMPONENTS_SPLIT) return bad(err, MRCNN_ERR_SHAPE, "%s: unknown mode %d", who, q.mode);
    if (q.mode == MRCNN_COMPONENTS_SPLIT && s.of != MRCNN_COMPONENTS_OF_ONES)
        return bad(err, MRCNN_ERR_SHAPE, "%s: MRCNN_COMPONENTS_SPLIT cuts components of ones only (of = %d)", who, s.of);
    if (q.n_comps < 0) return bad(err, MRCNN_ERR_SHAPE, "%s: n_comps %lld is negative", who, (long long)q.n_comps);
    if (!q.out_run_offsets || !q.out_n || (!q.keep && q.n_comps > 0) || (!q.out_parent && q.mode == MRCNN_COMPONENTS_SPLIT))
        return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (q.capacity < 0 || (!q.out_counts && q.capacity != 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null out_counts with capacity %lld", who, (long long)q.capacity);
    return MRCNN_OK;
}

int bad_comp_capacity(long long need, long long capacity, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: the set has %lld components, the component arrays hold %lld: call again with comp_capacity >= %lld", who, need,
               capacity, need);
}

int bad_n_comps(long long given, long long found, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: keep holds n_comps = %lld entries, the set has %lld components", who, given, found);
}

namespace {

// One RLE labelled: its plane (column-major: pixel (y, x) at x*h + y), the component of every pixel of the labelled value (-1 elsewhere)
// and the pixels of every component, in the order the flood met them.
struct Labelled {
    int h, w;
    std::vector<uint8_t> plane;
    std::vector<int32_t> label;
    std::vector<std::vector<uint32_t>> pixels;
};

void label_rle(const Set& s, int64_t k, Labelled& L)
{
    const int h = L.h = s.heights[k], w = L.w = s.widths[k];
    const size_t hw = (size_t)h * w;
    const int conn = components_connectivity(s.connectivity, s.of);
    L.plane.assign(hw, 0); L.label.assign(hw, -1); L.pixels.clear();
    size_t p = 0;
    for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
        const uint32_t c = s.counts[j];
        if ((j - s.run_offsets[k]) & 1) std::fill(L.plane.begin() + (ptrdiff_t)p, L.plane.begin() + (ptrdiff_t)(p + c), (uint8_t)1);
        p += c;
    }
    std::vector<uint32_t> stack;
    for (size_t seed = 0; seed < hw; ++seed) {                   // rising position: a component is numbered by its first pixel
        if (L.plane[seed] != (uint8_t)s.of || L.label[seed] >= 0) continue;
        const int32_t id = (int32_t)L.pixels.size();
        L.pixels.emplace_back();
        std::vector<uint32_t>& mine = L.pixels.back();
        L.label[seed] = id;
        stack.push_back((uint32_t)seed);
        while (!stack.empty()) {
            const uint32_t q = stack.back();
            stack.pop_back();
            mine.push_back(q);
            const int x = (int)(q / (uint32_t)h), y = (int)(q % (uint32_t)h);
            for (int dx = -1; dx <= 1; ++dx)
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((!dx && !dy) || (conn == 4 && dx && dy)) continue;
                    const int nx = x + dx, ny = y + dy;
                    if (nx < 0 || nx >= w || ny < 0 || ny >= h) continue;        // nothing continues outside the image
                    const size_t t = (size_t)nx * h + ny;
                    if (L.plane[t] != (uint8_t)s.of || L.label[t] >= 0) continue;
                    L.label[t] = id;
                    stack.push_back((uint32_t)t);
                }
        }
    }
}

struct Encoded { std::vector<uint32_t> runs; uint32_t area; int32_t box[4]; };

struct Encoder {
    Encoded& e; int h; size_t hw;
    size_t at = 0;                                               // pixels encoded so far
    int xmin, ymin, xmax = -1, ymax = -1;
    uint8_t cur = 0; size_t start = 0;
    Encoder(Encoded& enc, int h_, int w_) : e(enc), h(h_), hw((size_t)h_ * w_), xmin(w_), ymin(h_) { e.area = 0; }
    void put(uint8_t v, size_t n)                                // n pixels of value v follow
    {
        if (!n) return;
        if (v != cur) { e.runs.push_back((uint32_t)(at - start)); start = at; cur = v; }
        if (v) {
            e.area += (uint32_t)n;
            const int x0 = (int)(at / (size_t)h), x1 = (int)((at + n - 1) / (size_t)h);
            xmin = std::min(xmin, x0); xmax = std::max(xmax, x1);
            if (x0 != x1) { ymin = 0; ymax = h - 1; }
            else { ymin = std::min(ymin, (int)(at % (size_t)h)); ymax = std::max(ymax, (int)((at + n - 1) % (size_t)h)); }
        }
        at += n;
    }
    void finish()                                                // what was not put is 0
    {
        put(0, hw - at);
        e.runs.push_back((uint32_t)(hw - start));
        const bool any = e.area > 0;
        e.box[0] = any ? xmin : 0; e.box[1] = any ? ymin : 0; e.box[2] = any ? xmax - xmin + 1 : 0; e.box[3] = any ? ymax - ymin + 1 : 0;
    }
};

}  // namespace

int components_host(const Set& s, const Measures& m, std::string* err)
{
    const char* who = "rle_components_host";
    int st = check_measures(s, m, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    std::vector<uint32_t> areas;
    std::vector<int32_t> boxes;
    std::vector<uint8_t> flags;
    std::vector<int64_t> offs((size_t)s.n + 1, 0);
    Labelled L;
    for (int64_t k = 0; k < s.n; ++k) {
        label_rle(s, k, L);
        for (const std::vector<uint32_t>& px : L.pixels) {
            int xmin = L.w, ymin = L.h, xmax = -1, ymax = -1;
            for (const uint32_t q : px) {
                const int x = (int)(q / (uint32_t)L.h), y = (int)(q % (uint32_t)L.h);
                xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
            }
            areas.push_back((uint32_t)px.size());
            boxes.insert(boxes.end(), {xmin, ymin, xmax - xmin + 1, ymax - ymin + 1});
            flags.push_back((uint8_t)(xmin == 0 || ymin == 0 || xmax == L.w - 1 || ymax == L.h - 1));
        }
        offs[(size_t)k + 1] = (int64_t)areas.size();
    }
    std::copy(offs.begin(), offs.end(), m.comp_offsets);
    const long long need = (long long)areas.size();
    if (need > (long long)m.comp_capacity) return bad_comp_capacity(need, (long long)m.comp_capacity, who, err);
    std::copy(areas.begin(), areas.end(), m.comp_areas);
    std::copy(boxes.begin(), boxes.end(), m.comp_bboxes_xywh);
    std::copy(flags.begin(), flags.end(), m.comp_flags);
    return MRCNN_OK;
}

int select_host(const Set& s, const Select& q, std::string* err)
{
    const char* who = "rle_components_select_host";
    int st = check_select(s, q, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    // pass 1 only counts, so that n_comps is judged before anything is written; pass 2 labels again: one plane at a time is held
    Labelled L;
    long long found = 0;
    for (int64_t k = 0; k < s.n; ++k) {
        label_rle(s, k, L);
        found += (long long)L.pixels.size();
    }
    if (found != (long long)q.n_comps) return bad_n_comps((long long)q.n_comps, found, who, err);

    std::vector<Encoded> done;
    std::vector<int64_t> parent;
    long long c0 = 0;
    for (int64_t k = 0; k < s.n; ++k) {
        label_rle(s, k, L);
        const size_t hw = (size_t)L.h * L.w;
        if (q.mode == MRCNN_COMPONENTS_MERGE) {
            done.emplace_back();
            Encoder enc(done.back(), L.h, L.w);
            for (size_t p = 0; p < hw; ++p) {
                const int32_t c = L.label[p];
                enc.put(c < 0 ? L.plane[p] : (uint8_t)(q.keep[c0 + c] ? s.of : !s.of), 1);
            }
            enc.finish();
            parent.push_back(k);
        } else {
            for (size_t c = 0; c < L.pixels.size(); ++c) {
                if (!q.keep[c0 + (long long)c]) continue;
                done.emplace_back();
                Encoder enc(done.back(), L.h, L.w);
                std::sort(L.pixels[c].begin(), L.pixels[c].end());              // rising position: the encoder's order
                for (const uint32_t p : L.pixels[c]) { enc.put(0, (size_t)p - enc.at); enc.put(1, 1); }
                enc.finish();
                parent.push_back(k);
            }
        }
        c0 += (long long)L.pixels.size();
    }

    // everything but the runs is written whatever the capacity; the runs only when all of them fit
    const size_t m = done.size();
    long long need = 0;
    q.out_run_offsets[0] = 0;
    for (size_t j = 0; j < m; ++j) {
        need += (long long)done[j].runs.size();
        q.out_run_offsets[j + 1] = need;
        if (q.areas) q.areas[j] = done[j].area;
        if (q.bboxes_xywh) std::copy(done[j].box, done[j].box + 4, q.bboxes_xywh + 4 * j);
        if (q.out_parent) q.out_parent[j] = parent[j];
    }
    *q.out_n = (int64_t)m;
    if (need > (long long)q.capacity) return rle_set::bad_runs_capacity(need, (long long)q.capacity, who, err);
    for (size_t j = 0; j < m; ++j) std::copy(done[j].runs.begin(), done[j].runs.end(), q.out_counts + q.out_run_offsets[j]);
    return MRCNN_OK;
}

}  // namespace rle_components
}  // namespace mrcnn
