// polygons_host.cpp — see polygons_host.h.  The obvious tracer, sequential and plain on purpose: this file is what the kernels of
// kernels_polygons.hip are compared with.  Decode the plane with a border of unset pixels; visit the vertices in the order of
// polygon_rule.h (x, then y); an unvisited boundary edge that leaves a vertex starts a ring there — every ring through a smaller vertex
// has been walked by then, so the vertex is the ring's smallest — and the ring is walked edge by edge until it closes.
#include "polygons_host.h"

#include <algorithm>

#include "polygon_rule.h"

namespace mrcnn {
namespace polygons {

int check_arguments(const rle_draw::Set& s, const int64_t* rle_rings, const int64_t* n_rings, const int64_t* n_vertices, const int64_t* ring_offsets,
                    int64_t ring_capacity, const int32_t* xy, int64_t vertex_capacity, const char* who, std::string* err)
{
    const int st = rle_draw::check_set(s, 0x7fffffff, who, err);
    if (st != MRCNN_OK) return st;
    if (!rle_rings || !n_rings || !n_vertices) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (ring_capacity < 0 || vertex_capacity < 0)
        return bad(err, MRCNN_ERR_INVALID, "%s: capacities %lld rings, %lld vertices: neither may be negative", who, (long long)ring_capacity,
                   (long long)vertex_capacity);
    if (!ring_offsets && ring_capacity > 0) return bad(err, MRCNN_ERR_INVALID, "%s: null ring_offsets with a capacity of %lld rings", who, (long long)ring_capacity);
    if (!xy && vertex_capacity > 0) return bad(err, MRCNN_ERR_INVALID, "%s: null xy with a capacity of %lld vertices", who, (long long)vertex_capacity);
    return MRCNN_OK;
}

int check_capacity(int64_t rings, int64_t vertices, int64_t ring_capacity, int64_t vertex_capacity, const char* who, std::string* err)
{
    if (rings > ring_capacity || vertices > vertex_capacity)
        return bad(err, MRCNN_ERR_SHAPE, "%s: the set traces to %lld rings of %lld vertices, the buffers hold %lld rings and %lld vertices: call again "
                   "with ring_capacity >= %lld and vertex_capacity >= %lld", who, (long long)rings, (long long)vertices, (long long)ring_capacity,
                   (long long)vertex_capacity, (long long)rings, (long long)vertices);
    return MRCNN_OK;
}

namespace {

// one h x w plane inside a border of unset pixels, and which of the four edges that leave a vertex have been walked
struct Plane {
    int h, w;
    std::vector<uint8_t> px, walked;
    Plane(int h_, int w_) : h(h_), w(w_), px((size_t)(h_ + 2) * (w_ + 2), 0), walked((size_t)(h_ + 1) * (w_ + 1), 0) {}
    uint8_t& at(int x, int y) { return px[(size_t)(y + 1) * (w + 2) + (x + 1)]; }              // -1 <= x <= w, -1 <= y <= h
    PolyNbhd round(int X, int Y) { return PolyNbhd{at(X - 1, Y - 1), at(X, Y - 1), at(X - 1, Y), at(X, Y)}; }
    uint8_t& edges(int X, int Y) { return walked[(size_t)Y * (w + 1) + X]; }
};

// the ring that leaves (X, Y) with heading d: its corners behind out->xy, its offset and its area
void walk(Plane& p, int X, int Y, int d, Rings* out)
{
    const size_t first = out->xy.size();
    out->xy.push_back(X); out->xy.push_back(Y);                  // the smallest vertex of a ring is a corner: nothing of the ring lies left of it
    int x = X, y = Y, heading = d;
    for (;;) {
        p.edges(x, y) |= (uint8_t)(1 << heading);
        x += poly_dx(heading); y += poly_dy(heading);
        const int next = poly_turn(heading, p.round(x, y));
        if (x == X && y == Y && next == d) break;                // closed
        if (next != heading) { out->xy.push_back(x); out->xy.push_back(y); }
        heading = next;
    }
    const size_t m = (out->xy.size() - first) / 2;
    const int32_t* v = out->xy.data() + first;
    int64_t twice = 0;                                           // sum of x_i*y_{i+1} - x_{i+1}*y_i: even, the edges are axis-parallel
    for (size_t i = 0; i < m; ++i) {
        const size_t j = i + 1 < m ? i + 1 : 0;
        twice += (int64_t)v[2 * i] * v[2 * j + 1] - (int64_t)v[2 * j] * v[2 * i + 1];
    }
    out->ring_areas.push_back(twice / 2);
    out->ring_offsets.push_back((int64_t)(out->xy.size() / 2));
}

}  // namespace

int trace_host(const rle_draw::Set& s, const char* who, Rings* out, std::string* err)
{
    const int st = rle_draw::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;
    const int64_t n = (int64_t)s.n_images * s.slots;
    Rings r;
    r.rle_rings.assign(1, 0);
    r.ring_offsets.assign(1, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int b = (int)(k / s.slots);
        const int h = s.heights[b], w = s.widths[b];
        Plane p(h, w);
        uint32_t pos = 0;
        int x_lo = w, x_hi = -1;                                 // the pixel columns that hold a set pixel
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
            const uint32_t c = s.counts[j];
            if ((j - s.run_offsets[k]) & 1)
                for (uint32_t q = pos; q < pos + c; ++q) {       // a run that crosses a column end simply goes on at the top of the next column
                    const int x = (int)(q / (uint32_t)h);
                    p.at(x, (int)(q % (uint32_t)h)) = 1;
                    x_lo = std::min(x_lo, x); x_hi = std::max(x_hi, x);
                }
            pos += c;
        }
        for (int X = x_lo; X <= x_hi + 1; ++X)                   // (no boundary edge leaves a vertex outside these columns)
            for (int Y = 0; Y <= h; ++Y) {
                const PolyNbhd nb = p.round(X, Y);
                for (int d = 0; d < 4; ++d)
                    if (poly_out_edge(d, nb) && !(p.edges(X, Y) & (1 << d))) walk(p, X, Y, d, &r);
            }
        r.rle_rings.push_back((int64_t)r.ring_areas.size());
    }
    *out = std::move(r);
    return MRCNN_OK;
}

}  // namespace polygons
}  // namespace mrcnn
