// rle_shape_host.cpp — see rle_shape_host.h.  The rules of include/maskrcnn_hip.h as they read, sequential and plain on purpose: this
// file is what the kernels of kernels_rle_shape.hip are compared with.
#include "rle_shape_host.h"

#include <algorithm>

#include "shape_rule.h"

namespace mrcnn {
namespace rle_shape {

int check_hull_arguments(const int64_t* hull_offsets, const int32_t* xy, const int64_t* n_vertices, int64_t vertex_capacity, const char* who,
                         std::string* err)
{
    if (!hull_offsets || !n_vertices) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    if (vertex_capacity < 0) return bad(err, MRCNN_ERR_INVALID, "%s: vertex_capacity %lld is negative", who, (long long)vertex_capacity);
    if (!xy && vertex_capacity > 0) return bad(err, MRCNN_ERR_INVALID, "%s: null xy with a capacity of %lld vertices", who, (long long)vertex_capacity);
    return MRCNN_OK;
}

int bad_capacity(long long need, long long capacity, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: the hulls have %lld vertices, xy holds %lld: call again with vertex_capacity >= %lld", who, need, capacity, need);
}

namespace {

// The column pieces of RLE k: rows [a, b) of pixel column x, touching pieces of one column joined, in column-major order; first[x] ..
// first[x + 1] are column x's.
struct Piece { int a, b; };
struct Pieces { std::vector<Piece> p; std::vector<size_t> first; };

void cut(const Set& s, int64_t k, Pieces* out)
{
    const int h = s.heights[k], w = s.widths[k];
    out->p.clear();
    out->first.assign((size_t)w + 1, 0);
    std::vector<int> col;                                        // the column of every piece
    uint64_t pos = 0;
    for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) {
        const uint64_t n = s.counts[j];
        if ((j - s.run_offsets[k]) & 1) {
            for (uint64_t at = pos; at < pos + n;) {             // one piece per column the run touches
                const int x = (int)(at / (uint64_t)h), a = (int)(at % (uint64_t)h);
                const int b = (int)std::min<uint64_t>((uint64_t)h, a + (pos + n - at));
                if (!col.empty() && col.back() == x && out->p.back().b == a) out->p.back().b = b;       // (a zero-length run of zeros lay between)
                else { out->p.push_back(Piece{a, b}); col.push_back(x); }
                at += (uint64_t)(b - a);
            }
        }
        pos += n;
    }
    size_t i = 0;
    for (int x = 0; x <= w; ++x) {
        while (i < col.size() && col[i] < x) ++i;
        out->first[(size_t)x] = i;
    }
}

// the rows in which two columns' pieces differ
int64_t differ(const Piece* A, size_t na, const Piece* B, size_t nb)
{
    int64_t len = 0, both = 0;
    for (size_t i = 0; i < na; ++i) len += A[i].b - A[i].a;
    for (size_t i = 0; i < nb; ++i) len += B[i].b - B[i].a;
    for (size_t i = 0, j = 0; i < na && j < nb;) {
        const int lo = std::max(A[i].a, B[j].a), hi = std::min(A[i].b, B[j].b);
        if (hi > lo) both += hi - lo;
        if (A[i].b <= B[j].b) ++i; else ++j;
    }
    return len - 2 * both;
}

}  // namespace

int measure_host(const Set& s, int64_t* measures, std::string* err)
{
    const char* who = "rle_measure_host";
    int st = rle_set::check_flat(s, who, err);
    if (st != MRCNN_OK) return st;
    if (!measures && s.n > 0) return bad(err, MRCNN_ERR_INVALID, "%s: null measures", who);
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;
    Pieces P;
    for (int64_t k = 0; k < s.n; ++k) {
        const int w = s.widths[k];
        cut(s, k, &P);
        int64_t* m = measures + SHAPE_MEASURE_WORDS * k;
        std::fill(m, m + SHAPE_MEASURE_WORDS, (int64_t)0);
        for (int x = 0; x < w; ++x)
            for (size_t i = P.first[(size_t)x]; i < P.first[(size_t)x + 1]; ++i)
                for (int64_t y = P.p[i].a; y < P.p[i].b; ++y) {
                    m[0] += 1; m[1] += x; m[2] += y;
                    m[3] += (int64_t)x * x; m[4] += (int64_t)x * y; m[5] += y * y;
                }
        // the unit edges: between pixel columns X - 1 and X where exactly one is set (the outside is unset), and above and below every piece
        for (int X = 0; X <= w; ++X) {
            const size_t a0 = X > 0 ? P.first[(size_t)X - 1] : 0, a1 = X > 0 ? P.first[(size_t)X] : 0;
            const size_t b0 = X < w ? P.first[(size_t)X] : 0, b1 = X < w ? P.first[(size_t)X + 1] : 0;
            m[6] += differ(P.p.data() + a0, a1 - a0, P.p.data() + b0, b1 - b0) + 2 * (int64_t)(b1 - b0);
        }
    }
    return MRCNN_OK;
}

int convex_hull_host(const Set& s, int64_t* hull_offsets, int64_t* hull_areas2, int64_t* obb, int32_t* xy, int64_t* n_vertices, int64_t vertex_capacity,
                     std::string* err)
{
    const char* who = "rle_convex_hull_host";
    int st = rle_set::check_flat(s, who, err);
    if (st != MRCNN_OK) return st;
    st = check_hull_arguments(hull_offsets, xy, n_vertices, vertex_capacity, who, err);
    if (st != MRCNN_OK) return st;
    st = rle_set::check_sums(s, who, err);
    if (st != MRCNN_OK) return st;

    Pieces P;
    std::vector<int32_t> all;                                    // the rings back to back: x, y per vertex
    std::vector<int> ring, T, B;
    hull_offsets[0] = 0;
    for (int64_t k = 0; k < s.n; ++k) {
        const int w = s.widths[k];
        cut(s, k, &P);
        // the candidates of every vertex column: the extremes of its non-empty neighbours
        T.assign((size_t)w + 1, -1); B.assign((size_t)w + 1, -1);
        for (int x = 0; x < w; ++x) {
            if (P.first[(size_t)x] == P.first[(size_t)x + 1]) continue;
            const int t = P.p[P.first[(size_t)x]].a, b = P.p[P.first[(size_t)x + 1] - 1].b;
            for (int X = x; X <= x + 1; ++X) {
                T[(size_t)X] = T[(size_t)X] < 0 ? t : std::min(T[(size_t)X], t);
                B[(size_t)X] = std::max(B[(size_t)X], b);
            }
        }
        // Andrew's monotone chain in walking order: a vertex stays only while it lies strictly left of the chord around it
        ring.clear();
        const auto chain = [&](size_t from, int X, int Y) {
            while (ring.size() >= from + 4) {
                const size_t q = ring.size();
                if (shape_cross(ring[q - 4], ring[q - 3], X, Y, ring[q - 2], ring[q - 1]) > 0) break;
                ring.resize(q - 2);
            }
            ring.push_back(X); ring.push_back(Y);
        };
        for (int X = 0; X <= w; ++X) if (T[(size_t)X] >= 0) chain(0, X, T[(size_t)X]);
        const size_t top = ring.size();
        for (int X = w; X >= 0; --X) if (B[(size_t)X] >= 0) chain(top, X, B[(size_t)X]);
        const int m = (int)(ring.size() / 2);
        hull_offsets[k + 1] = hull_offsets[k] + m;

        const auto X = [&](int i) { return ring[2 * (size_t)i]; };
        const auto Y = [&](int i) { return ring[2 * (size_t)i + 1]; };
        if (hull_areas2) {
            int64_t a2 = 0;
            for (int i = 0; i < m; ++i) {
                const int j = i + 1 < m ? i + 1 : 0;
                a2 += (int64_t)X(i) * Y(j) - (int64_t)X(j) * Y(i);
            }
            hull_areas2[k] = a2;
        }
        if (obb) {
            int64_t* o = obb + SHAPE_OBB_WORDS * k;
            std::fill(o, o + SHAPE_OBB_WORDS, (int64_t)0);
            o[0] = -1;
            ShapeScore best{};
            for (int e = 0; e < m; ++e) {
                const ShapeBox b = shape_edge_box(m, e, X, Y);
                const ShapeScore sc = shape_score(b);
                if (e > 0 && !shape_box_before(sc, e, best, (int)o[0])) continue;
                best = sc;
                o[0] = e; o[1] = b.dx; o[2] = b.dy; o[3] = b.dmin; o[4] = b.dmax; o[5] = b.cmin; o[6] = b.cmax;
            }
        }
        all.insert(all.end(), ring.begin(), ring.end());
    }
    const long long need = (long long)(all.size() / 2);
    *n_vertices = need;
    if (need > (long long)vertex_capacity) return bad_capacity(need, (long long)vertex_capacity, who, err);
    if (need) std::copy(all.begin(), all.end(), xy);
    return MRCNN_OK;
}

}  // namespace rle_shape
}  // namespace mrcnn
