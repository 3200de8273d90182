// nest_host.cpp — see nest_host.h.  The rule of nest_rule.h as it reads, sequential and plain on purpose: this file is what the kernels
// of kernels_nest.hip are compared with.  Quadratic in the rings of an RLE, and meant to be.
#include "nest_host.h"

#include <utility>

#include "nest_rule.h"

namespace mrcnn {
namespace nest {

int check_arguments(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, const int64_t* parent,
                    const int32_t* depth, const int64_t* rle_polys, const int64_t* poly_rings, const int64_t* ring_order, const int64_t* n_polys,
                    const char* who, std::string* err)
{
    if (n_rles < 0) return bad(err, MRCNN_ERR_INVALID, "%s: n_rles %lld is negative", who, (long long)n_rles);
    if (n_rings < 0) return bad(err, MRCNN_ERR_INVALID, "%s: n_rings %lld is negative", who, (long long)n_rings);
    if (!rle_rings || !ring_offsets || !rle_polys || !poly_rings || !n_polys || ((!xy || !parent || !depth || !ring_order) && n_rings > 0))
        return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    return MRCNN_OK;
}

int bad_rle_rings(int64_t rle, int64_t n_rings, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: rle_rings does not start at 0, decreases or does not end at n_rings = %lld at RLE %lld", who, (long long)n_rings,
               (long long)rle);
}

int check_rle_rings(const int64_t* rle_rings, int64_t n_rles, int64_t n_rings, const char* who, std::string* err)
{
    if (rle_rings[0] != 0 || (n_rles == 0 && n_rings != 0)) return bad_rle_rings(0, n_rings, who, err);
    for (int64_t k = 0; k < n_rles; ++k)
        if (rle_rings[k + 1] < rle_rings[k] || (k == n_rles - 1 && rle_rings[k + 1] != n_rings)) return bad_rle_rings(k, n_rings, who, err);
    return MRCNN_OK;
}

namespace {

struct Ring {
    const int32_t* v;                                            // x then y per vertex
    int64_t m;
    int x(int64_t i) const { return v[2 * i]; }
    int y(int64_t i) const { return v[2 * i + 1]; }
};

int64_t area2(const Ring& r)
{
    int64_t twice = 0;
    for (int64_t i = 0; i < r.m; ++i) {
        const int64_t j = i + 1 < r.m ? i + 1 : 0;
        twice += nest_area_term(r.x(i), r.y(i), r.x(j), r.y(j));
    }
    return twice;
}

// contains(q, the ring whose first vertex is (X0, Y0))
bool contains(const Ring& q, int X0, int Y0)
{
    if (q.m < 3) return false;
    bool odd = false;
    for (int64_t i = 0; i < q.m; ++i) {
        const int64_t j = i + 1 < q.m ? i + 1 : 0;
        if (nest_crosses(q.x(i), q.y(i), q.x(j), q.y(j), X0, Y0)) odd = !odd;
    }
    return odd;
}

}  // namespace

void nest_host(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, Nest* out)
{
    const size_t n = (size_t)n_rings;
    const auto ring = [&](int64_t r) { return Ring{xy + 2 * ring_offsets[r], ring_offsets[r + 1] - ring_offsets[r]}; };
    std::vector<uint64_t> size(n);
    for (int64_t r = 0; r < n_rings; ++r) size[(size_t)r] = nest_abs(area2(ring(r)));

    Nest t;
    t.parent.assign(n, -1);
    for (int64_t k = 0; k < n_rles; ++k)
        for (int64_t r = rle_rings[k]; r < rle_rings[k + 1]; ++r) {
            const Ring me = ring(r);
            if (me.m == 0) continue;                             // no probe
            int64_t best = -1;
            for (int64_t q = rle_rings[k]; q < rle_rings[k + 1]; ++q) {
                if (q == r || !nest_outranks(size[(size_t)q], q, size[(size_t)r], r) || !contains(ring(q), me.x(0), me.y(0))) continue;
                if (best < 0 || nest_closer(size[(size_t)q], q, size[(size_t)best], best)) best = q;
            }
            t.parent[(size_t)r] = best;
        }

    t.depth.assign(n, 0);
    for (int64_t r = 0; r < n_rings; ++r)
        for (int64_t p = t.parent[(size_t)r]; p >= 0; p = t.parent[(size_t)p]) ++t.depth[(size_t)r];      // (a forest: the walk ends)

    std::vector<std::vector<int64_t>> holes(n);                  // per shell, in ring order
    for (int64_t r = 0; r < n_rings; ++r)
        if (t.depth[(size_t)r] & 1) holes[(size_t)t.parent[(size_t)r]].push_back(r);
    t.rle_polys.assign((size_t)n_rles + 1, 0);
    t.ring_order.reserve(n);
    for (int64_t k = 0; k < n_rles; ++k) {
        for (int64_t r = rle_rings[k]; r < rle_rings[k + 1]; ++r) {
            if (t.depth[(size_t)r] & 1) continue;
            t.poly_rings.push_back((int64_t)t.ring_order.size());
            t.ring_order.push_back(r);
            for (const int64_t h : holes[(size_t)r]) t.ring_order.push_back(h);
        }
        t.rle_polys[(size_t)k + 1] = (int64_t)t.poly_rings.size();
    }
    t.poly_rings.push_back((int64_t)t.ring_order.size());
    *out = std::move(t);
}

}  // namespace nest
}  // namespace mrcnn
