// tiles_host.cpp — see tiles_host.h.  Sequential and plain on purpose: this file is what the merge kernels are compared with.
#include "tiles_host.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace mrcnn {
namespace tiles {

// ---- the planner: one axis ---------------------------------------------------------------------
static int axis_count(int L, int T, int O) { return L <= T ? 1 : (L - T + (T - O) - 1) / (T - O) + 1; }
static int axis_origin(int L, int T, int O, int k) { return L <= T ? 0 : std::min(k * (T - O), L - T); }

int plan(int height, int width, int tile_h, int tile_w, int overlap_y, int overlap_x, int image, mrcnn_tile* out, int capacity, int* count,
         std::string* err)
{
    if (!count) return bad(err, MRCNN_ERR_INVALID, "tile_plan: null count");
    if (capacity < 0 || (!out && capacity != 0)) return bad(err, MRCNN_ERR_INVALID, "tile_plan: null out with capacity %d", capacity);
    if (height < 1 || height > 32767 || width < 1 || width > 32767)
        return bad(err, MRCNN_ERR_SHAPE, "tile_plan: the image is %dx%d: height and width must lie in 1..32767", height, width);
    if (tile_h < 1 || tile_h > 32767 || tile_w < 1 || tile_w > 32767)
        return bad(err, MRCNN_ERR_SHAPE, "tile_plan: the tile is %dx%d: height and width must lie in 1..32767", tile_h, tile_w);
    if (overlap_y < 0 || overlap_y >= tile_h || overlap_x < 0 || overlap_x >= tile_w)
        return bad(err, MRCNN_ERR_SHAPE, "tile_plan: overlap (%d, %d) must lie in 0..tile-1 of a %dx%d tile", overlap_y, overlap_x, tile_h, tile_w);
    const int ny = axis_count(height, tile_h, overlap_y), nx = axis_count(width, tile_w, overlap_x);
    const long need = (long)ny * nx;
    if (need > 0x7fffffffL) return bad(err, MRCNN_ERR_SHAPE, "tile_plan: %ld tiles are too many", need);
    *count = (int)need;
    if (!out) return MRCNN_OK;                                  // the size query
    if (need > capacity) return bad(err, MRCNN_ERR_SHAPE, "tile_plan: the plan has %ld tiles, out holds %d", need, capacity);
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            mrcnn_tile& t = out[(size_t)j * nx + i];
            t.image = image;
            t.y0 = axis_origin(height, tile_h, overlap_y, j); t.x0 = axis_origin(width, tile_w, overlap_x, i);
            t.height = std::min(tile_h, height); t.width = std::min(tile_w, width);
        }
    return MRCNN_OK;
}

// ---- argument checks -----------------------------------------------------------------------------
int check_tiles(const mrcnn_tile* tiles, int n_tiles, const int32_t* heights, const int32_t* widths, int n_images, const char* who, std::string* err)
{
    const int sides = check_sides(heights, widths, n_images, who, err);
    if (sides != MRCNN_OK) return sides;
    for (int t = 0; t < n_tiles; ++t) {
        const mrcnn_tile& w = tiles[t];
        if (w.image < 0 || w.image >= n_images) return bad(err, MRCNN_ERR_SHAPE, "%s: tile %d names image %d of %d", who, t, w.image, n_images);
        if (w.height < 1 || w.width < 1) return bad(err, MRCNN_ERR_SHAPE, "%s: tile %d is an empty window (%dx%d)", who, t, w.height, w.width);
        const int h = heights[w.image], wd = widths[w.image];
        if (w.y0 < 0 || w.x0 < 0 || w.y0 > h - w.height || w.x0 > wd - w.width)
            return bad(err, MRCNN_ERR_SHAPE, "%s: tile %d (%dx%d at %d,%d) is not inside image %d (%dx%d)", who, t, w.height, w.width, w.y0, w.x0,
                       w.image, h, wd);
    }
    return MRCNN_OK;
}

int check_merge(const MergeArgs& a, const char* who, std::string* err, const char* threshold)
{
    if (!a.detections || !a.masks || !a.tiles || !a.heights || !a.widths || !a.detections_src || !a.source || !a.n_kept || !a.run_offsets)
        return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (a.capacity < 0 || (!a.counts && a.capacity != 0)) return bad(err, MRCNN_ERR_INVALID, "%s: null counts with capacity %lld", who, (long long)a.capacity);
    if (a.mask_size < 2 || a.model_h < 1 || a.model_w < 1) return bad(err, MRCNN_ERR_INVALID, "%s: bad mask or model size", who);
    if (a.metric != MRCNN_MATCH_IOU && a.metric != MRCNN_MATCH_IOS) return bad(err, MRCNN_ERR_INVALID, "%s: metric %d is neither MRCNN_MATCH_IOU nor MRCNN_MATCH_IOS", who, a.metric);
    if (!(a.match_threshold > 0.0)) return bad(err, MRCNN_ERR_INVALID, "%s: %s %g must be > 0", who, threshold, a.match_threshold);
    if (a.n_tiles < 1) return bad(err, MRCNN_ERR_SHAPE, "%s: n_tiles %d < 1", who, a.n_tiles);
    if (a.n_images < 1 || a.rows < 1 || a.max_out < 1) return bad(err, MRCNN_ERR_SHAPE, "%s: n_images %d, rows %d and max_out %d must be >= 1", who, a.n_images, a.rows, a.max_out);
    if ((long)a.n_tiles * a.rows >= (1L << 31) || (long)a.n_images * a.max_out >= (1L << 31)) return bad(err, MRCNN_ERR_SHAPE, "%s: too many rows", who);
    const int st = check_tiles(a.tiles, a.n_tiles, a.heights, a.widths, a.n_images, who, err);
    if (st != MRCNN_OK) return st;
    std::vector<long> per((size_t)a.n_images, 0);
    for (int t = 0; t < a.n_tiles; ++t) per[(size_t)a.tiles[t].image] += a.rows;
    for (int b = 0; b < a.n_images; ++b)
        if (per[(size_t)b] > MRCNN_TILES_MAX_CANDIDATES)
            return bad(err, MRCNN_ERR_SHAPE, "%s: image %d has %ld candidates (tiles x rows), at most %d can be merged", who, b, per[(size_t)b], MRCNN_TILES_MAX_CANDIDATES);
    return MRCNN_OK;
}

// ---- the merge -----------------------------------------------------------------------------------
namespace {

struct Candidate {
    int box[4];                      // (y1, x1, y2, x2) in the full frame, far edges exclusive; all 0 = not eligible
    bool eligible;
    float row[6];                    // the source-frame row
    std::vector<uint32_t> counts;    // COCO RLE of the plane in the full frame
    uint32_t area;
    int bbox[4];
};

// paste_device.h's paste_tap / paste_lerp, operation for operation
struct Tap { int a, b; float f; };
Tap tap(int i, int lo, float scale, int S)
{
    float s = ((float)(i - lo) + 0.5f) * scale - 0.5f;
    s = fminf(fmaxf(s, 0.0f), (float)(S - 1));
    Tap t;
    t.a = (int)floorf(s); t.b = std::min(t.a + 1, S - 1);
    t.f = s - (float)t.a;
    return t;
}
float lerp2(float a, float b, float c, float dd, float fx, float fy)
{
    const float top = a + (b - a) * fx;
    const float bot = c + (dd - c) * fx;
    return top + (bot - top) * fy;
}

// the candidate's box: mrcnn_unletterbox_boxes on the tile's own size, denorm_boxes at that size, then the shift by the origin
void map_box(const float* d, const mrcnn_tile& t, int H, int W, int img_h, int img_w, Candidate& c)
{
    int nh = 0, nw = 0, py = 0, px = 0;
    mrcnn_letterbox_geometry(t.height, t.width, H, W, &nh, &nw, &py, &px);
    float r[4] = {d[0], d[1], d[2], d[3]};
    const int h = t.height, w = t.width;
    if (!(r[0] == 0.f && r[1] == 0.f && r[2] == 0.f && r[3] == 0.f)) {
        const double sy = (double)h / nh, sx = (double)w / nw, hy = h > 1 ? h - 1 : 1, wx = w > 1 ? w - 1 : 1;
        const double y1 = ((double)r[0] * (H - 1) - py) * sy, x1 = ((double)r[1] * (W - 1) - px) * sx;
        const double y2 = ((double)r[2] * (H - 1) + 1.0 - py) * sy, x2 = ((double)r[3] * (W - 1) + 1.0 - px) * sx;
        auto clip = [](double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); };
        r[0] = (float)clip(y1 / hy); r[1] = (float)clip(x1 / wx); r[2] = (float)clip((y2 - 1.0) / hy); r[3] = (float)clip((x2 - 1.0) / wx);
    }
    const int by1 = (int)rint((double)r[0] * (double)(h - 1)), bx1 = (int)rint((double)r[1] * (double)(w - 1));
    const int by2 = (int)rint((double)r[2] * (double)(h - 1) + 1.0), bx2 = (int)rint((double)r[3] * (double)(w - 1) + 1.0);
    c.eligible = !(by2 - by1 <= 0 || bx2 - bx1 <= 0 || !(d[5] > 0.0f));
    for (int k = 0; k < 6; ++k) c.row[k] = 0.f;
    c.box[0] = c.box[1] = c.box[2] = c.box[3] = 0;
    if (!c.eligible) return;
    c.box[0] = by1 + t.y0; c.box[1] = bx1 + t.x0; c.box[2] = by2 + t.y0; c.box[3] = bx2 + t.x0;
    const double hy = img_h > 1 ? img_h - 1 : 1, wx = img_w > 1 ? img_w - 1 : 1;
    c.row[0] = (float)((double)c.box[0] / hy); c.row[1] = (float)((double)c.box[1] / wx);
    c.row[2] = (float)((double)(c.box[2] - 1) / hy); c.row[3] = (float)((double)(c.box[3] - 1) / wx);
    c.row[4] = d[4]; c.row[5] = d[5];
}

// the plane in the full frame as COCO runs: positions p = x*h + y in increasing order, only the box can hold set pixels
void encode(const float* m, int S, float thr, int h, int w, Candidate& c)
{
    c.counts.clear(); c.area = 0;
    c.bbox[0] = c.bbox[1] = c.bbox[2] = c.bbox[3] = 0;
    const long total = (long)h * w;
    long cursor = 0, start = -1, end = -1;         // [start, end): the run of ones being grown
    int xmin = w, ymin = h, xmax = -1, ymax = -1;
    auto close = [&] {
        if (start < 0) return;
        c.counts.push_back((uint32_t)(start - cursor)); c.counts.push_back((uint32_t)(end - start));
        cursor = end; start = -1;
    };
    if (c.eligible) {
        const int y1 = c.box[0], x1 = c.box[1], y2 = c.box[2], x2 = c.box[3];
        const float sy = (float)S / (float)(y2 - y1), sx = (float)S / (float)(x2 - x1);
        for (int x = x1; x < x2; ++x) {
            const Tap tx = tap(x, x1, sx, S);
            for (int y = y1; y < y2; ++y) {
                const Tap ty = tap(y, y1, sy, S);
                const float *ra = m + ty.a * S, *rb = m + ty.b * S;
                if (!(lerp2(ra[tx.a], ra[tx.b], rb[tx.a], rb[tx.b], tx.f, ty.f) >= thr)) continue;
                const long p = (long)x * h + y;
                if (start >= 0 && p == end) ++end; else { close(); start = p; end = p + 1; }
                ++c.area;
                xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
            }
        }
    }
    close();
    if (c.counts.empty() || cursor < total) c.counts.push_back((uint32_t)(total - cursor));
    if (c.area) { c.bbox[0] = xmin; c.bbox[1] = ymin; c.bbox[2] = xmax - xmin + 1; c.bbox[3] = ymax - ymin + 1; }
}

// |A ∧ B| of two RLEs over the same number of pixels
uint64_t intersection(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b)
{
    uint64_t inter = 0, pa = 0, pb = 0;      // the ends of run ia / ib
    size_t ia = 0, ib = 0;
    if (a.empty() || b.empty()) return 0;
    pa = a[0]; pb = b[0];
    uint64_t at = 0;
    while (ia < a.size() && ib < b.size()) {
        const uint64_t to = std::min(pa, pb);
        if ((ia & 1) && (ib & 1)) inter += to - at;
        at = to;
        if (pa == to) { ++ia; if (ia < a.size()) pa += a[ia]; }
        if (pb == to) { ++ib; if (ib < b.size()) pb += b[ib]; }
    }
    return inter;
}

double measure(uint64_t inter, uint64_t aq, uint64_t ac, int metric)
{
    const uint64_t den = metric == MRCNN_MATCH_IOU ? aq + ac - inter : std::min(aq, ac);
    return den == 0 ? 0.0 : (double)inter / (double)den;
}

}  // namespace

namespace {

// the candidates of a call: box, eligibility, source-frame row and plane of every row of every tile
std::vector<Candidate> candidates(const MergeArgs& a)
{
    const int S = a.mask_size;
    std::vector<Candidate> cand((size_t)a.n_tiles * a.rows);
    for (int t = 0; t < a.n_tiles; ++t)
        for (int i = 0; i < a.rows; ++i) {
            const long k = (long)t * a.rows + i;
            const mrcnn_tile& w = a.tiles[t];
            map_box(a.detections + k * 6, w, a.model_h, a.model_w, a.heights[w.image], a.widths[w.image], cand[(size_t)k]);
            encode(a.masks + k * S * S, S, a.threshold, a.heights[w.image], a.widths[w.image], cand[(size_t)k]);
        }
    return cand;
}

// the eligible candidates of image b by (score descending, k ascending)
std::vector<long> image_order(const MergeArgs& a, const std::vector<Candidate>& cand, int b)
{
    std::vector<long> order;
    for (long k = 0; k < (long)cand.size(); ++k)
        if (a.tiles[k / a.rows].image == b && cand[(size_t)k].eligible) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](long p, long q) { return cand[(size_t)p].row[5] > cand[(size_t)q].row[5]; });
    return order;
}

void clear_slots(const MergeArgs& a)
{
    const long slots = (long)a.n_images * a.max_out;
    for (long s = 0; s < slots; ++s) {
        a.source[s] = -1;
        for (int k = 0; k < 6; ++k) a.detections_src[s * 6 + k] = 0.f;
    }
}

// the planes of the slots in mrcnn_masks_rle_source's layout; a padding slot (nullptr) is the empty plane of its image
int emit(const MergeArgs& a, const char* who, const std::vector<const Candidate*>& plane, std::string* err)
{
    const long slots = (long)a.n_images * a.max_out;
    int64_t need = 0;
    for (long s = 0; s < slots; ++s) {
        const Candidate* c = plane[(size_t)s];
        a.run_offsets[s] = need;
        need += c ? (int64_t)c->counts.size() : 1;
        if (a.areas) a.areas[s] = c ? c->area : 0;
        if (a.bboxes_xywh) for (int k = 0; k < 4; ++k) a.bboxes_xywh[s * 4 + k] = c ? c->bbox[k] : 0;
    }
    a.run_offsets[slots] = need;
    if (need > a.capacity)
        return bad(err, MRCNN_ERR_SHAPE, "%s: the kept masks encode to %lld runs, counts holds %lld: call again with capacity >= %lld", who,
                   (long long)need, (long long)a.capacity, (long long)need);
    for (long s = 0; s < slots; ++s) {
        uint32_t* o = a.counts + a.run_offsets[s];
        if (plane[(size_t)s]) std::copy(plane[(size_t)s]->counts.begin(), plane[(size_t)s]->counts.end(), o);
        else { const int b = (int)(s / a.max_out); o[0] = (uint32_t)a.heights[b] * (uint32_t)a.widths[b]; }
    }
    return MRCNN_OK;
}

}  // namespace

int merge_host(const MergeArgs& a, std::string* err)
{
    const int st = check_merge(a, "merge_tiles_host", err);
    if (st != MRCNN_OK) return st;
    const std::vector<Candidate> cand = candidates(a);
    clear_slots(a);
    std::vector<const Candidate*> plane((size_t)a.n_images * a.max_out, nullptr);
    for (int b = 0; b < a.n_images; ++b) {
        const std::vector<long> order = image_order(a, cand, b);
        std::vector<long> kept;
        for (long c : order) {
            const Candidate& cc = cand[(size_t)c];
            bool dropped = false;
            for (long q : kept) {
                const Candidate& cq = cand[(size_t)q];
                if (cq.row[4] != cc.row[4] || q / a.rows == c / a.rows) continue;
                if (measure(intersection(cq.counts, cc.counts), cq.area, cc.area, a.metric) >= a.match_threshold) { dropped = true; break; }
            }
            if (!dropped) kept.push_back(c);
        }
        a.n_kept[b] = (int32_t)kept.size();
        for (size_t j = 0; j < kept.size() && j < (size_t)a.max_out; ++j) {
            const long s = (long)b * a.max_out + (long)j;
            a.source[s] = (int32_t)kept[j];
            for (int k = 0; k < 6; ++k) a.detections_src[s * 6 + k] = cand[(size_t)kept[j]].row[k];
            plane[(size_t)s] = &cand[(size_t)kept[j]];
        }
    }
    return emit(a, "merge_tiles_host", plane, err);
}

// ---- uniting -------------------------------------------------------------------------------------
namespace {

struct Rect { int y0, x0, y1, x1; };                // rows [y0, y1), columns [x0, x1)

// the positions p < n of a plane of height h (p = x*h + y) that lie inside r
int64_t inside(const Rect& r, int h, uint32_t n)
{
    const int64_t x = n / (uint32_t)h, y = n % (uint32_t)h, rw = r.x1 - r.x0, rh = r.y1 - r.y0;
    const int64_t full = std::min(std::max(x - r.x0, (int64_t)0), rw);
    const int64_t part = (x >= r.x0 && x < r.x1) ? std::min(std::max(y - r.y0, (int64_t)0), rh) : 0;
    return full * rh + part;
}

// one walk over two run lists of the same plane: |A ∧ B|, |A ∧ R|, |B ∧ R|
void clipped(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const Rect& r, int h, uint64_t* inter, uint64_t* ar, uint64_t* br)
{
    *inter = *ar = *br = 0;
    if (a.empty() || b.empty()) return;
    uint64_t pa = a[0], pb = b[0], at = 0;
    int64_t fat = 0;
    size_t ia = 0, ib = 0;
    while (ia < a.size() && ib < b.size()) {
        const uint64_t to = std::min(pa, pb);
        const int64_t fto = inside(r, h, (uint32_t)to);
        if (ia & 1) *ar += (uint64_t)(fto - fat);
        if (ib & 1) *br += (uint64_t)(fto - fat);
        if ((ia & 1) && (ib & 1)) *inter += to - at;
        at = to; fat = fto;
        if (pa == to) { ++ia; if (ia < a.size()) pa += a[ia]; }
        if (pb == to) { ++ib; if (ib < b.size()) pb += b[ib]; }
    }
}

bool linked(const MergeArgs& a, const std::vector<Candidate>& cand, long q, long c)
{
    const Candidate &cq = cand[(size_t)q], &cc = cand[(size_t)c];
    if (cq.row[4] != cc.row[4] || q / a.rows == c / a.rows) return false;
    const mrcnn_tile &tq = a.tiles[q / a.rows], &tc = a.tiles[c / a.rows];
    const Rect r = {std::max(tq.y0, tc.y0), std::max(tq.x0, tc.x0), std::min(tq.y0 + tq.height, tc.y0 + tc.height),
                    std::min(tq.x0 + tq.width, tc.x0 + tc.width)};
    if (r.y1 <= r.y0 || r.x1 <= r.x0) return false;
    uint64_t inter, aq, ac;
    clipped(cq.counts, cc.counts, r, a.heights[tq.image], &inter, &aq, &ac);
    return measure(inter, aq, ac, a.metric) >= a.match_threshold;
}

// the OR of the members' planes; a run one member ends where another begins is one run
void unite(const std::vector<Candidate>& cand, const std::vector<long>& members, long total, Candidate& u)
{
    std::vector<std::pair<uint32_t, uint32_t>> ones;            // [start, end) of every run of ones of every member
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (long k : members) {
        const Candidate& c = cand[(size_t)k];
        uint32_t p = 0;
        for (size_t i = 0; i < c.counts.size(); ++i) {
            if ((i & 1) && c.counts[i]) ones.push_back({p, p + c.counts[i]});
            p += c.counts[i];
        }
        if (c.area) {                                           // the tight box of a union is the hull of the tight boxes
            x0 = std::min(x0, c.bbox[0]); y0 = std::min(y0, c.bbox[1]);
            x1 = std::max(x1, c.bbox[0] + c.bbox[2]); y1 = std::max(y1, c.bbox[1] + c.bbox[3]);
        }
    }
    std::sort(ones.begin(), ones.end());
    u.counts.clear(); u.area = 0;
    uint32_t cursor = 0;
    for (size_t i = 0; i < ones.size();) {
        uint32_t s = ones[i].first, e = ones[i].second;
        for (++i; i < ones.size() && ones[i].first <= e; ++i) e = std::max(e, ones[i].second);
        u.counts.push_back(s - cursor); u.counts.push_back(e - s);
        u.area += e - s; cursor = e;
    }
    if (u.counts.empty() || (long)cursor < total) u.counts.push_back((uint32_t)(total - cursor));
    u.bbox[0] = u.bbox[1] = u.bbox[2] = u.bbox[3] = 0;
    if (u.area) { u.bbox[0] = x0; u.bbox[1] = y0; u.bbox[2] = x1 - x0; u.bbox[3] = y1 - y0; }
}

}  // namespace

int unite_host(const MergeArgs& a, std::string* err)
{
    const int st = check_merge(a, "unite_tiles_host", err, "link_threshold");
    if (st != MRCNN_OK) return st;
    const std::vector<Candidate> cand = candidates(a);
    const long slots = (long)a.n_images * a.max_out;
    clear_slots(a);
    if (a.n_parts) for (long s = 0; s < slots; ++s) a.n_parts[s] = 0;
    if (a.group) for (size_t k = 0; k < cand.size(); ++k) a.group[k] = -1;
    std::vector<Candidate> united((size_t)slots);
    std::vector<const Candidate*> plane((size_t)slots, nullptr);
    for (int b = 0; b < a.n_images; ++b) {
        const std::vector<long> order = image_order(a, cand, b);
        const size_t n = order.size();
        std::vector<size_t> label(n);                           // the least place of the component, by union-find on places
        for (size_t r = 0; r < n; ++r) label[r] = r;
        auto find = [&](size_t r) { while (label[r] != r) r = label[r] = label[label[r]]; return r; };
        for (size_t rc = 1; rc < n; ++rc)
            for (size_t rq = 0; rq < rc; ++rq)
                if (linked(a, cand, order[rq], order[rc])) {
                    const size_t x = find(rq), y = find(rc);
                    if (x != y) label[std::max(x, y)] = std::min(x, y);
                }
        std::vector<std::vector<long>> members;                 // by the representative's place; members in place order
        std::vector<long> index(n, -1);
        for (size_t r = 0; r < n; ++r) {
            const size_t rep = find(r);
            if (rep == r) { index[r] = (long)members.size(); members.emplace_back(); }
            members[(size_t)index[rep]].push_back(order[r]);
            if (a.group) a.group[order[r]] = (int32_t)index[rep];
        }
        a.n_kept[b] = (int32_t)members.size();
        const double hy = a.heights[b] > 1 ? a.heights[b] - 1 : 1, wx = a.widths[b] > 1 ? a.widths[b] - 1 : 1;
        for (size_t j = 0; j < members.size() && j < (size_t)a.max_out; ++j) {
            const long s = (long)b * a.max_out + (long)j;
            const Candidate& rep = cand[(size_t)members[j][0]];
            int hull[4] = {rep.box[0], rep.box[1], rep.box[2], rep.box[3]};
            for (long k : members[j]) {
                const int* bx = cand[(size_t)k].box;
                hull[0] = std::min(hull[0], bx[0]); hull[1] = std::min(hull[1], bx[1]); hull[2] = std::max(hull[2], bx[2]); hull[3] = std::max(hull[3], bx[3]);
            }
            float* o = a.detections_src + s * 6;
            o[0] = (float)((double)hull[0] / hy); o[1] = (float)((double)hull[1] / wx);
            o[2] = (float)((double)(hull[2] - 1) / hy); o[3] = (float)((double)(hull[3] - 1) / wx);
            o[4] = rep.row[4]; o[5] = rep.row[5];
            a.source[s] = (int32_t)members[j][0];
            if (a.n_parts) a.n_parts[s] = (int32_t)members[j].size();
            unite(cand, members[j], (long)a.heights[b] * a.widths[b], united[(size_t)s]);
            plane[(size_t)s] = &united[(size_t)s];
        }
    }
    return emit(a, "unite_tiles_host", plane, err);
}

}  // namespace tiles
}  // namespace mrcnn
