// simplify_host.cpp — see simplify_host.h.  Douglas-Peucker as it is usually written, sequential and plain on purpose: this file is
// what the kernels of kernels_simplify.hip are compared with.  A ring's two anchors are found, its two chains go on a stack, and a chain
// that keeps its chosen vertex puts its two halves there.
#include "simplify_host.h"

#include <cmath>
#include <utility>

#include "simplify_rule.h"

namespace mrcnn {
namespace simplify {

int check_arguments(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, double tolerance, const int64_t* out_ring_offsets,
                    const int32_t* out_xy, const int64_t* n_vertices_out, int64_t vertex_capacity, const char* who, std::string* err)
{
    if (n_rings < 0) return bad(err, MRCNN_ERR_INVALID, "%s: n_rings %lld is negative", who, (long long)n_rings);
    if (!ring_offsets || !out_ring_offsets || !n_vertices_out || (!xy && n_rings > 0)) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (!(tolerance >= 0.0 && tolerance <= SIMP_TOLERANCE_MAX))                              // (NaN fails both)
        return bad(err, MRCNN_ERR_INVALID, "%s: tolerance %g is not a number in 0..65535", who, tolerance);
    if (vertex_capacity < 0) return bad(err, MRCNN_ERR_INVALID, "%s: vertex_capacity %lld is negative", who, (long long)vertex_capacity);
    if (!out_xy && vertex_capacity > 0) return bad(err, MRCNN_ERR_INVALID, "%s: null out_xy with a capacity of %lld vertices", who, (long long)vertex_capacity);
    return MRCNN_OK;
}

int bad_offsets(int64_t ring, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: ring_offsets are negative, decrease or span 2^31 vertices or more at ring %lld", who, (long long)ring);
}

int bad_coordinate(int64_t ring, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: ring %lld has a coordinate outside 0..%d", who, (long long)ring, SIMP_COORD_MAX);
}

int check_offsets(const int64_t* ring_offsets, int64_t n_rings, const char* who, std::string* err, int64_t* most)
{
    *most = 0;
    for (int64_t r = 0; r < n_rings; ++r) {
        const int64_t m = ring_offsets[r + 1] - ring_offsets[r];
        if (ring_offsets[r] < 0 || ring_offsets[r + 1] < ring_offsets[r] || m >= (1LL << 31)) return bad_offsets(r, who, err);
        if (m > *most) *most = m;
    }
    return MRCNN_OK;
}

int check_coordinates(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, const char* who, std::string* err)
{
    for (int64_t r = 0; r < n_rings; ++r)
        for (int64_t v = 2 * ring_offsets[r]; v < 2 * ring_offsets[r + 1]; ++v)
            if (xy[v] < 0 || xy[v] > SIMP_COORD_MAX) return bad_coordinate(r, who, err);
    return MRCNN_OK;
}

int check_capacity(int64_t vertices, int64_t vertex_capacity, const char* who, std::string* err)
{
    if (vertices > vertex_capacity)
        return bad(err, MRCNN_ERR_SHAPE, "%s: the rings simplify to %lld vertices, the buffers hold %lld: call again with vertex_capacity >= %lld", who,
                   (long long)vertices, (long long)vertex_capacity, (long long)vertices);
    return MRCNN_OK;
}

namespace {

// one ring of m >= 3 vertices at v: keep[i] = 1 for the vertices that stay
void simplify_ring(const int32_t* v, int m, uint64_t E, std::vector<uint8_t>& keep, std::vector<std::pair<int, int>>& stack)
{
    const auto X = [&](int i) { return (int)v[2 * (i == m ? 0 : i)]; };
    const auto Y = [&](int i) { return (int)v[2 * (i == m ? 0 : i) + 1]; };
    keep.assign((size_t)m, 0);
    int f = 0;
    uint32_t far = 0;
    for (int i = 1; i < m; ++i) {
        const uint32_t d = simp_dist2(X(0), Y(0), X(i), Y(i));
        if (d > far) { far = d; f = i; }                         // (strictly: the smallest index on a tie)
    }
    keep[0] = 1; keep[(size_t)f] = 1;
    stack.clear();
    stack.emplace_back(0, f);
    stack.emplace_back(f, m);
    while (!stack.empty()) {
        const int a = stack.back().first, b = stack.back().second;
        stack.pop_back();
        if (b - a < 2) continue;
        int k = a + 1;
        uint32_t c = simp_distance(X(a), Y(a), X(b), Y(b), X(k), Y(k));
        for (int i = a + 2; i < b; ++i) {
            const uint32_t ci = simp_distance(X(a), Y(a), X(b), Y(b), X(i), Y(i));
            if (ci > c) { c = ci; k = i; }
        }
        if (!simp_keeps(c, E, X(a), Y(a), X(b), Y(b))) continue;     // every vertex strictly between a and b is dropped
        keep[(size_t)k] = 1;
        stack.emplace_back(a, k);
        stack.emplace_back(k, b);
    }
}

}  // namespace

void simplify_host(const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, uint64_t E, Rings* out)
{
    Rings r;
    r.ring_offsets.assign(1, 0);
    std::vector<uint8_t> keep;
    std::vector<std::pair<int, int>> stack;
    for (int64_t q = 0; q < n_rings; ++q) {
        const int64_t v0 = ring_offsets[q];
        const int m = (int)(ring_offsets[q + 1] - v0);
        if (m <= 2) keep.assign((size_t)m, 1);
        else simplify_ring(xy + 2 * v0, m, E, keep, stack);
        const size_t first = r.xy.size() / 2;
        for (int i = 0; i < m; ++i)
            if (keep[(size_t)i]) {
                r.xy.push_back(xy[2 * (v0 + i)]); r.xy.push_back(xy[2 * (v0 + i) + 1]);
                r.src_index.push_back(v0 + i);
            }
        const size_t n = r.xy.size() / 2 - first;
        const int32_t* v = r.xy.data() + 2 * first;
        int64_t twice = 0;                                       // sum of x_i*y_{i+1} - x_{i+1}*y_i round the simplified ring
        for (size_t i = 0; i < n; ++i) {
            const size_t j = i + 1 < n ? i + 1 : 0;
            twice += (int64_t)v[2 * i] * v[2 * j + 1] - (int64_t)v[2 * j] * v[2 * i + 1];
        }
        r.areas2.push_back(twice);
        r.ring_offsets.push_back((int64_t)(r.xy.size() / 2));
    }
    *out = std::move(r);
}

}  // namespace simplify
}  // namespace mrcnn
