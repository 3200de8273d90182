// rle_draw_host.cpp — see rle_draw_host.h.  The obvious painter, sequential and plain on purpose: this file is what the kernels of
// kernels_rle_draw.hip are compared with.  Decode the runs, lowest row first; a pixel keeps its first owner.
#include "rle_draw_host.h"

#include <algorithm>
#include <vector>

#include "draw_rule.h"
#include "rle_set_host.h"

namespace mrcnn {
namespace rle_draw {

// ---- argument checks -----------------------------------------------------------------------------
int check_set(const Set& s, int max_slots, const char* who, std::string* err)
{
    if (!s.run_offsets || !s.heights || !s.widths) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (s.n_images < 0 || s.slots < 0) return bad(err, MRCNN_ERR_INVALID, "%s: n_images %d, slots %d: neither may be negative", who, s.n_images, s.slots);
    if (s.slots > max_slots) return bad(err, MRCNN_ERR_SHAPE, "%s: %d slots are too many (at most %d)", who, s.slots, max_slots);
    if ((int64_t)s.n_images * s.slots >= (1LL << 31)) return bad(err, MRCNN_ERR_SHAPE, "%s: %d x %d RLEs are too many", who, s.n_images, s.slots);
    return check_sides(s.heights, s.widths, s.n_images, who, err);
}

int check_render(int alpha, int stroke, const char* who, std::string* err)
{
    if (alpha < 0 || alpha > 256) return bad(err, MRCNN_ERR_SHAPE, "%s: alpha %d outside 0..256", who, alpha);
    if (stroke < 0 || stroke > 65534) return bad(err, MRCNN_ERR_SHAPE, "%s: stroke %d outside 0..65534", who, stroke);
    return MRCNN_OK;
}

int bad_sum(const Set& s, int64_t k, unsigned long long sum, const char* who, std::string* err)
{
    const int b = (int)(k / s.slots);
    return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld (image %d, slot %d) sums to %llu pixels, its %dx%d plane has %llu", who, (long long)k, b, (int)(k % s.slots),
               sum, s.heights[b], s.widths[b], (unsigned long long)s.heights[b] * (unsigned long long)s.widths[b]);
}

// every RLE sums to its plane, or nothing is drawn
int check_sums(const Set& s, const char* who, std::string* err)
{
    const int64_t n = (int64_t)s.n_images * s.slots;
    int st = rle_set::check_run_offsets(s.run_offsets, n, who, err);
    if (st == MRCNN_OK) st = rle_set::check_counts(s.counts, s.run_offsets, n, who, err);
    if (st != MRCNN_OK) return st;
    for (int64_t k = 0; k < n; ++k) {
        const int b = (int)(k / s.slots);
        uint64_t sum = 0;
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) sum += s.counts[j];
        if (sum != (uint64_t)s.heights[b] * (uint64_t)s.widths[b]) return bad_sum(s, k, sum, who, err);
    }
    return MRCNN_OK;
}

// calls set(y, x) for every set pixel of RLE k, in run order
template <class F>
static void for_each_set(const Set& s, int64_t k, int h, F&& set)
{
    uint32_t p = 0;
    for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
        const uint32_t c = s.counts[j];
        if ((j - s.run_offsets[k]) & 1)
            for (uint32_t q = p; q < p + c; ++q) set((int)(q % (uint32_t)h), (int)(q / (uint32_t)h));
        p += c;
    }
}

// ---- the definitions -----------------------------------------------------------------------------
int decode_host(const Set& s, uint8_t* out, const int64_t* out_offsets, std::string* err)
{
    int st = check_set(s, 0x7fffffff, "rle_decode_host", err);
    if (st != MRCNN_OK) return st;
    if (!out) return bad(err, MRCNN_ERR_INVALID, "rle_decode_host: null out");
    st = check_offsets(s.heights, s.widths, s.n_images, out_offsets, s.slots, "rle_decode_host", nullptr, err);
    if (st != MRCNN_OK) return st;
    st = check_sums(s, "rle_decode_host", err);
    if (st != MRCNN_OK) return st;
    for (int b = 0; b < s.n_images; ++b) {
        const int h = s.heights[b], w = s.widths[b];
        for (int i = 0; i < s.slots; ++i) {
            uint8_t* const plane = out + out_offsets[b] + (int64_t)i * h * w;
            std::fill(plane, plane + (size_t)h * w, (uint8_t)0);
            for_each_set(s, (int64_t)b * s.slots + i, h, [&](int y, int x) { plane[(size_t)y * w + x] = 1; });
        }
    }
    return MRCNN_OK;
}

// the owners of one image: the lowest drawn row whose plane is set, -1 for none
static void paint_owners(const Set& s, const float* det, float min_score, int b, int16_t* own, uint32_t* visible)
{
    const int h = s.heights[b], w = s.widths[b];
    std::fill(own, own + (size_t)h * w, (int16_t)-1);
    for (int i = 0; i < s.slots; ++i) {
        if (visible) visible[i] = 0;
        const float* row = det + ((size_t)b * s.slots + i) * 6;
        if (!rle_draw_drawn(row, rle_draw_box(row, h, w), min_score)) continue;
        uint32_t mine = 0;
        for_each_set(s, (int64_t)b * s.slots + i, h, [&](int y, int x) {
            int16_t& o = own[(size_t)y * w + x];
            if (o < 0) { o = (int16_t)i; ++mine; }
        });
        if (visible) visible[i] = mine;
    }
}

int instance_map_host(const Set& s, const float* detections_src, float min_score, int16_t* map, const int64_t* map_offsets, uint32_t* visible_areas,
                      std::string* err)
{
    int st = check_set(s, 32767, "instance_map_rle_host", err);
    if (st != MRCNN_OK) return st;
    if (!detections_src || !map) return bad(err, MRCNN_ERR_INVALID, "instance_map_rle_host: null argument");
    if (reinterpret_cast<uintptr_t>(map) % 2 != 0) return bad(err, MRCNN_ERR_INVALID, "instance_map_rle_host: map is not aligned for int16");
    st = check_offsets(s.heights, s.widths, s.n_images, map_offsets, 2, "instance_map_rle_host", nullptr, err);
    if (st != MRCNN_OK) return st;
    st = check_sums(s, "instance_map_rle_host", err);
    if (st != MRCNN_OK) return st;
    for (int b = 0; b < s.n_images; ++b)
        paint_owners(s, detections_src, min_score, b, reinterpret_cast<int16_t*>(reinterpret_cast<uint8_t*>(map) + map_offsets[b]),
                     visible_areas ? visible_areas + (size_t)b * s.slots : nullptr);
    return MRCNN_OK;
}

int render_host(const Set& s, const mrcnn_image* images, const float* detections_src, float min_score, int alpha, int stroke, uint8_t* out_rgb,
                const int64_t* out_offsets, std::string* err)
{
    if (!images) return bad(err, MRCNN_ERR_INVALID, "render_detections_rle_host: null images");
    std::vector<int32_t> hs((size_t)std::max(s.n_images, 0)), ws(hs.size());
    for (int b = 0; b < s.n_images; ++b) {
        if (!images[b].rgb) return bad(err, MRCNN_ERR_INVALID, "render_detections_rle_host: image %d has a null rgb pointer", b);
        hs[(size_t)b] = images[b].height; ws[(size_t)b] = images[b].width;
    }
    Set t = s;
    t.heights = hs.data(); t.widths = ws.data();
    int st = check_set(t, 32767, "render_detections_rle_host", err);
    if (st != MRCNN_OK) return st;
    if (!detections_src || !out_rgb) return bad(err, MRCNN_ERR_INVALID, "render_detections_rle_host: null argument");
    st = check_render(alpha, stroke, "render_detections_rle_host", err);
    if (st != MRCNN_OK) return st;
    st = check_offsets(t.heights, t.widths, t.n_images, out_offsets, 3, "render_detections_rle_host", nullptr, err);
    if (st != MRCNN_OK) return st;
    st = check_sums(t, "render_detections_rle_host", err);
    if (st != MRCNN_OK) return st;
    const int grow = stroke / 2, shrink = stroke - stroke / 2;
    std::vector<int16_t> own, ring;
    for (int b = 0; b < t.n_images; ++b) {
        const int h = hs[(size_t)b], w = ws[(size_t)b];
        own.resize((size_t)h * w); ring.assign((size_t)h * w, (int16_t)-1);
        paint_owners(t, detections_src, min_score, b, own.data(), nullptr);
        for (int i = 0; i < t.slots && stroke > 0; ++i) {
            const float* row = detections_src + ((size_t)b * t.slots + i) * 6;
            const RleDrawBox box = rle_draw_box(row, h, w);
            if (!rle_draw_drawn(row, box, min_score)) continue;
            for (int y = std::max(0, box.y1 - grow); y < std::min(h, box.y2 + grow); ++y)
                for (int x = std::max(0, box.x1 - grow); x < std::min(w, box.x2 + grow); ++x)
                    if (ring[(size_t)y * w + x] < 0 && in_ring(box, grow, shrink, y, x)) ring[(size_t)y * w + x] = (int16_t)i;
        }
        const uint8_t* src = images[b].rgb;
        uint8_t* out = out_rgb + out_offsets[b];
        for (size_t p = 0; p < (size_t)h * w; ++p) {
            for (int ch = 0; ch < 3; ++ch) out[p * 3 + ch] = (uint8_t)render_byte(src[p * 3 + ch], pixel_code(own[p], ring[p]), ch, alpha);
        }
    }
    return MRCNN_OK;
}

}  // namespace rle_draw
}  // namespace mrcnn
