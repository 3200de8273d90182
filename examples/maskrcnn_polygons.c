/*
 * maskrcnn_polygons.c — run-length masks handed on as geometry, in plain C99 over include/maskrcnn_hip.h: an RLE set is read from a
 * text file, mrcnn_rle_to_polygons traces the boundary of every mask on the GPU (the size query first, then the call), and the rings
 * are printed, one per line, with their signed areas: positive for an outline, negative for a hole.  With --tolerance T the rings are
 * simplified first (mrcnn_polygons_simplify, Douglas-Peucker within T pixels): the areas printed stay the pixel areas.  With
 * --geojson FILE the traced rings are nested into outlines and their holes (mrcnn_polygons_nest) and FILE receives a GeoJSON
 * FeatureCollection: one Feature per mask that has a ring, a Polygon for one outline and a MultiPolygon for several, every hole with the
 * outline it lies in.  The nesting is that of the traced rings; a tolerance only changes the vertices written.  With --fill-holes the
 * holes of every mask are filled and with --min-area A its specks of fewer than A pixels are cleared before anything is traced, holes
 * first (mrcnn_rle_components measures the connected components, mrcnn_rle_components_select merges the kept ones back).  With
 * --disjoint every mask then loses the pixels of the masks before it in its image, so that no pixel belongs to two of them: one call of
 * mrcnn_rle_combine, group k = RLE k and the RLEs of its image before it, MRCNN_RLE_DIFF.  With --props the final masks are measured
 * (mrcnn_rle_measure, mrcnn_rle_convex_hull) and one line per mask that has a set pixel follows the rings: area, perimeter, centroid,
 * orientation, solidity and the four corners of the minimum-area oriented box; --geojson then writes the same as properties.
 *
 *   cc -std=c99 -Iinclude examples/maskrcnn_polygons.c -Lmask-rcnn-coreml_amd -lmaskrcnn_hip \
 *      -Wl,-rpath,$PWD/mask-rcnn-coreml_amd -Wl,-rpath-link,/opt/rocm/lib -o maskrcnn_polygons
 *   ./maskrcnn_polygons [--host] [--tolerance T] [--geojson FILE] [--props] [--min-area A] [--fill-holes] [--disjoint] <set.txt>
 *   (the flags in this order; --props, --min-area, --fill-holes and --disjoint in any)
 *
 * <set.txt> holds whitespace-separated integers: n_images and slots; then per image its height and width and, for each of its `slots`
 * RLEs, the number of runs followed by the runs (column-major, the first run counts zeros) — the layout mrcnn_masks_rle_source,
 * mrcnn_merge_tiles and mrcnn_unite_tiles write.  --host calls the sequential definitions, mrcnn_rle_to_polygons_host and
 * mrcnn_polygons_simplify_host (and mrcnn_polygons_nest_host, mrcnn_rle_components_host,
 * mrcnn_rle_components_select_host, mrcnn_rle_combine_host, mrcnn_rle_measure_host, mrcnn_rle_convex_hull_host), which need no GPU.  Exit status 0 on success; on failure the mrcnn_last_error() text goes to stderr and the status code is the exit status.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "maskrcnn_hip.h"

static int trace(int host, const uint32_t* counts, const int64_t* run_offsets, int n_images, int slots, const int32_t* heights, const int32_t* widths,
                 int64_t* rle_rings, int64_t* n_rings, int64_t* n_vertices, int64_t* ring_offsets, int64_t* ring_areas, int64_t ring_capacity,
                 int32_t* xy, int64_t vertex_capacity)
{
    if (host)
        return mrcnn_rle_to_polygons_host(counts, run_offsets, n_images, slots, heights, widths, rle_rings, n_rings, n_vertices, ring_offsets, ring_areas,
                                          ring_capacity, xy, vertex_capacity);
    return mrcnn_rle_to_polygons(counts, run_offsets, n_images, slots, heights, widths, MRCNN_HOST, rle_rings, n_rings, n_vertices, ring_offsets,
                                 ring_areas, ring_capacity, xy, vertex_capacity);
}

/* The set with some connected components of the value `of` merged away: those of fewer than min_area pixels (of ones), or those that do
 * not touch the image border (of zeros: the holes).  Both entries are asked for their sizes first.  *counts and run_offsets are replaced. */
static int filter_components(int host, int of, uint32_t** counts, int64_t* run_offsets, int64_t n, const int32_t* hs, const int32_t* ws, long long min_area)
{
    int64_t* comp_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t* out_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    uint32_t *areas = NULL, *out = NULL;
    int32_t* boxes = NULL;
    uint8_t *flags = NULL, *keep = NULL;
    int64_t comps = 0, runs = 0, out_n = 0;
    int st = -1;                                                 /* -1: out of memory, no library text goes with it */
    if (!comp_offsets || !out_offsets) goto done;
    comp_offsets[n] = 0;
    st = host ? mrcnn_rle_components_host(*counts, run_offsets, n, hs, ws, 4, of, comp_offsets, NULL, NULL, NULL, 0)
              : mrcnn_rle_components(*counts, run_offsets, n, hs, ws, 4, of, MRCNN_HOST, comp_offsets, NULL, NULL, NULL, 0);
    if (st != MRCNN_OK && !(st == MRCNN_ERR_SHAPE && comp_offsets[n] > 0)) goto done;
    comps = comp_offsets[n];
    areas = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(comps + 1));
    boxes = (int32_t*)malloc(sizeof(int32_t) * 4 * (size_t)(comps + 1));
    flags = (uint8_t*)malloc((size_t)(comps + 1));
    keep = (uint8_t*)malloc((size_t)(comps + 1));
    st = -1;
    if (!areas || !boxes || !flags || !keep) goto done;
    st = host ? mrcnn_rle_components_host(*counts, run_offsets, n, hs, ws, 4, of, comp_offsets, areas, boxes, flags, comps)
              : mrcnn_rle_components(*counts, run_offsets, n, hs, ws, 4, of, MRCNN_HOST, comp_offsets, areas, boxes, flags, comps);
    if (st != MRCNN_OK) goto done;
    for (int64_t c = 0; c < comps; ++c) keep[c] = of == MRCNN_COMPONENTS_OF_ONES ? (long long)areas[c] >= min_area : (flags[c] & 1) != 0;
    out_offsets[n] = 0;
    st = host ? mrcnn_rle_components_select_host(*counts, run_offsets, n, hs, ws, 4, of, keep, comps, MRCNN_COMPONENTS_MERGE, NULL, 0, out_offsets, NULL, NULL,
                                                 NULL, &out_n)
              : mrcnn_rle_components_select(*counts, run_offsets, n, hs, ws, 4, of, keep, comps, MRCNN_COMPONENTS_MERGE, MRCNN_HOST, NULL, 0, out_offsets, NULL,
                                            NULL, NULL, &out_n);
    if (st != MRCNN_OK && !(st == MRCNN_ERR_SHAPE && out_offsets[n] > 0)) goto done;
    runs = out_offsets[n];
    out = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(runs + 1));
    st = -1;
    if (!out) goto done;
    st = host ? mrcnn_rle_components_select_host(*counts, run_offsets, n, hs, ws, 4, of, keep, comps, MRCNN_COMPONENTS_MERGE, out, runs, out_offsets, NULL, NULL,
                                                 NULL, &out_n)
              : mrcnn_rle_components_select(*counts, run_offsets, n, hs, ws, 4, of, keep, comps, MRCNN_COMPONENTS_MERGE, MRCNN_HOST, out, runs, out_offsets, NULL,
                                            NULL, NULL, &out_n);
    if (st != MRCNN_OK) goto done;
    memcpy(run_offsets, out_offsets, sizeof(int64_t) * (size_t)(n + 1));
    free(*counts);
    *counts = out;
    out = NULL;
done:
    free(out); free(keep); free(flags); free(boxes); free(areas); free(out_offsets); free(comp_offsets);
    return st;
}

/* Every RLE minus the RLEs before it in its image: one call of mrcnn_rle_combine (after its size query) whatever the number of masks.
 * Group k lists RLE k first and then its image's RLEs before it; MRCNN_RLE_DIFF keeps what is set in the first member alone.  *counts
 * and run_offsets are replaced. */
static int make_disjoint(int host, uint32_t** counts, int64_t* run_offsets, int n_images, int slots, const int32_t* hs, const int32_t* ws)
{
    const int64_t n = (int64_t)n_images * slots, n_members = (int64_t)n_images * ((int64_t)slots * (slots + 1) / 2);
    int64_t* group_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t* members = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_members + 1));
    int64_t* out_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    uint32_t* out = NULL;
    int64_t at = 0, runs = 0;
    int st = -1;                                                 /* -1: out of memory, no library text goes with it */
    if (!group_offsets || !members || !out_offsets) goto done;
    group_offsets[0] = 0;
    for (int b = 0; b < n_images; ++b)
        for (int i = 0; i < slots; ++i) {
            const int64_t k = (int64_t)b * slots + i;
            members[at++] = k;
            for (int j = 0; j < i; ++j) members[at++] = (int64_t)b * slots + j;
            group_offsets[k + 1] = at;
        }
    out_offsets[n] = 0;
    st = host ? mrcnn_rle_combine_host(*counts, run_offsets, n, hs, ws, group_offsets, members, n, MRCNN_RLE_DIFF, NULL, 0, out_offsets, NULL, NULL)
              : mrcnn_rle_combine(*counts, run_offsets, n, hs, ws, group_offsets, members, n, MRCNN_RLE_DIFF, MRCNN_HOST, NULL, 0, out_offsets, NULL, NULL);
    if (st != MRCNN_OK && !(st == MRCNN_ERR_SHAPE && out_offsets[n] > 0)) goto done;
    runs = out_offsets[n];
    out = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(runs + 1));
    st = -1;
    if (!out) goto done;
    st = host ? mrcnn_rle_combine_host(*counts, run_offsets, n, hs, ws, group_offsets, members, n, MRCNN_RLE_DIFF, out, runs, out_offsets, NULL, NULL)
              : mrcnn_rle_combine(*counts, run_offsets, n, hs, ws, group_offsets, members, n, MRCNN_RLE_DIFF, MRCNN_HOST, out, runs, out_offsets, NULL, NULL);
    if (st != MRCNN_OK) goto done;
    memcpy(run_offsets, out_offsets, sizeof(int64_t) * (size_t)(n + 1));
    free(*counts);
    *counts = out;
    out = NULL;
done:
    free(out); free(out_offsets); free(members); free(group_offsets);
    return st;
}

/* What --props shows of one mask, in doubles made from the library's integers. */
typedef struct { int any; long long area, perimeter; double cx, cy, orientation, solidity, obb[8]; } mask_props;

/* atan2 in plain C (the example links against the library alone, not libm): the argument is brought to 0..1, then to within 1/8 of
 * one of five tabulated tangents, and the odd series of what is left converges in ten terms. */
static double angle_of(double y, double x)
{
    static const double tangent[5] = {0.0, 0.25, 0.5, 0.75, 1.0};
    static const double angle[5] = {0.0, 0.24497866312686414, 0.4636476090008061, 0.6435011087932844, 0.7853981633974483};
    const double pi = 3.141592653589793, ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
    if (ax == 0 && ay == 0) return 0.0;
    const int swap = ay > ax;
    const double t = swap ? ax / ay : ay / ax;
    const int c = (int)(t * 4.0 + 0.5);
    const double u = (t - tangent[c]) / (1.0 + t * tangent[c]), u2 = u * u;
    double sum = 0.0, term = u;
    for (int k = 0; k < 12; ++k) { sum += term / (2 * k + 1); term = -term * u2; }
    double a = angle[c] + sum;
    if (swap) a = pi / 2 - a;
    if (x < 0) a = pi - a;
    return y < 0 ? -a : a;
}

/* Measures, hulls and oriented boxes of the set (the hulls after a size query), then the doubles.  The central moments do not fit 64
 * bits as S1*Sxx - Sx^2: they are taken about the integer part of the mean, which is exact in int64, and corrected by the remainder. */
static int measure_props(int host, const uint32_t* counts, const int64_t* run_offsets, int64_t n, const int32_t* hs, const int32_t* ws, mask_props* out)
{
    int64_t* m = (int64_t*)malloc(sizeof(int64_t) * MRCNN_MEASURE_WORDS * (size_t)(n + 1));
    int64_t* hull_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t* areas2 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t* obb = (int64_t*)malloc(sizeof(int64_t) * 8 * (size_t)(n + 1));
    int32_t* xy = NULL;
    int64_t vertices = 0;
    int st = -1;                                                 /* -1: out of memory, no library text goes with it */
    if (!m || !hull_offsets || !areas2 || !obb) goto done;
    st = host ? mrcnn_rle_measure_host(counts, run_offsets, n, hs, ws, m) : mrcnn_rle_measure(counts, run_offsets, n, hs, ws, MRCNN_HOST, m);
    if (st != MRCNN_OK) goto done;
    st = host ? mrcnn_rle_convex_hull_host(counts, run_offsets, n, hs, ws, hull_offsets, NULL, NULL, NULL, &vertices, 0)
              : mrcnn_rle_convex_hull(counts, run_offsets, n, hs, ws, MRCNN_HOST, hull_offsets, NULL, NULL, NULL, &vertices, 0);
    if (st != MRCNN_OK && !(st == MRCNN_ERR_SHAPE && vertices > 0)) goto done;
    xy = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(vertices + 1));
    st = -1;
    if (!xy) goto done;
    st = host ? mrcnn_rle_convex_hull_host(counts, run_offsets, n, hs, ws, hull_offsets, areas2, obb, xy, &vertices, vertices)
              : mrcnn_rle_convex_hull(counts, run_offsets, n, hs, ws, MRCNN_HOST, hull_offsets, areas2, obb, xy, &vertices, vertices);
    if (st != MRCNN_OK) goto done;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t *w = m + MRCNN_MEASURE_WORDS * k, *o = obb + 8 * k;
        const int64_t s1 = w[0];
        mask_props* p = out + k;
        p->any = s1 > 0; p->area = (long long)s1; p->perimeter = (long long)w[6];
        if (!p->any) continue;
        const int64_t qx = w[1] / s1, rx = w[1] % s1, qy = w[2] / s1, ry = w[2] % s1;
        const double about_xx = (double)(w[3] - 2 * qx * w[1] + qx * qx * s1), about_yy = (double)(w[5] - 2 * qy * w[2] + qy * qy * s1);
        const double about_xy = (double)(w[4] - qx * w[2] - qy * w[1] + qx * qy * s1);
        const double c20 = (about_xx - (double)rx * (double)rx / (double)s1) / (double)s1 + 1.0 / 12.0;
        const double c02 = (about_yy - (double)ry * (double)ry / (double)s1) / (double)s1 + 1.0 / 12.0;
        const double c11 = (about_xy - (double)rx * (double)ry / (double)s1) / (double)s1;
        p->cx = (double)qx + (double)rx / (double)s1 + 0.5; p->cy = (double)qy + (double)ry / (double)s1 + 0.5;
        p->orientation = 0.5 * angle_of(2.0 * c11, c20 - c02);
        p->solidity = 2.0 * (double)s1 / (double)areas2[k];
        const double dx = (double)o[1], dy = (double)o[2], L2 = dx * dx + dy * dy;
        const double d[4] = {(double)o[3], (double)o[4], (double)o[4], (double)o[3]}, c[4] = {(double)o[5], (double)o[5], (double)o[6], (double)o[6]};
        for (int j = 0; j < 4; ++j) { p->obb[2 * j] = (d[j] * dx - c[j] * dy) / L2; p->obb[2 * j + 1] = (d[j] * dy + c[j] * dx) / L2; }
    }
done:
    free(xy); free(obb); free(areas2); free(hull_offsets); free(m);
    return st;
}

/* one ring as a closed GeoJSON ring: its first vertex repeated, an exterior with positive shoelace area and a hole with negative (a
 * traced ring has that already; a simplified one is reversed where it has not) */
static void write_ring(FILE* g, const int32_t* xy, int64_t v0, int64_t v1, int exterior)
{
    int64_t twice = 0;
    for (int64_t v = v0; v < v1; ++v) {
        const int64_t u = v + 1 < v1 ? v + 1 : v0;
        twice += (int64_t)xy[2 * v] * xy[2 * u + 1] - (int64_t)xy[2 * u] * xy[2 * v + 1];
    }
    const int reverse = twice != 0 && (twice < 0) == (exterior != 0);
    fprintf(g, "[[%d,%d]", (int)xy[2 * v0], (int)xy[2 * v0 + 1]);
    for (int64_t j = 1; j < v1 - v0; ++j) {
        const int64_t v = reverse ? v1 - j : v0 + j;
        fprintf(g, ",[%d,%d]", (int)xy[2 * v], (int)xy[2 * v + 1]);
    }
    fprintf(g, ",[%d,%d]]", (int)xy[2 * v0], (int)xy[2 * v0 + 1]);
}

/* The FeatureCollection of the set: polygon p owns ring_order[poly_rings[p] .. poly_rings[p+1]), its shell first; the polygons of RLE k
 * are [rle_polys[k], rle_polys[k+1]).  A shell with fewer than 3 vertices left is dropped with its holes, such a hole alone. */
static void write_geojson(FILE* g, size_t n, int slots, const int64_t* rle_rings, const int64_t* ring_offsets, const int64_t* ring_areas, const int32_t* xy,
                          const int64_t* rle_polys, const int64_t* poly_rings, const int64_t* ring_order, const mask_props* props)
{
    int features = 0;
    fprintf(g, "{\"type\":\"FeatureCollection\",\"features\":[");
    for (size_t k = 0; k < n; ++k) {
        int64_t shells = 0, area = 0;
        for (int64_t p = rle_polys[k]; p < rle_polys[k + 1]; ++p) {
            const int64_t s = ring_order[poly_rings[p]];
            shells += ring_offsets[s + 1] - ring_offsets[s] >= 3;
        }
        if (!shells) continue;
        for (int64_t r = rle_rings[k]; r < rle_rings[k + 1]; ++r) area += ring_areas[r];
        fprintf(g, "%s\n{\"type\":\"Feature\",\"geometry\":{\"type\":\"%s\",\"coordinates\":%s", features++ ? "," : "", shells > 1 ? "MultiPolygon" : "Polygon",
                shells > 1 ? "[" : "");
        int written = 0;
        for (int64_t p = rle_polys[k]; p < rle_polys[k + 1]; ++p) {
            const int64_t s = ring_order[poly_rings[p]];
            if (ring_offsets[s + 1] - ring_offsets[s] < 3) continue;
            fprintf(g, "%s[", written++ ? "," : "");
            write_ring(g, xy, ring_offsets[s], ring_offsets[s + 1], 1);
            for (int64_t j = poly_rings[p] + 1; j < poly_rings[p + 1]; ++j) {
                const int64_t h = ring_order[j];
                if (ring_offsets[h + 1] - ring_offsets[h] < 3) continue;
                fprintf(g, ",");
                write_ring(g, xy, ring_offsets[h], ring_offsets[h + 1], 0);
            }
            fprintf(g, "]");
        }
        fprintf(g, "%s},\"properties\":{\"image\":%d,\"row\":%d,\"area\":%lld", shells > 1 ? "]" : "", (int)(k / (size_t)slots), (int)(k % (size_t)slots),
                (long long)area);
        if (props && props[k].any) {
            const mask_props* p = props + k;
            fprintf(g, ",\"centroid\":[%.17g,%.17g],\"orientation\":%.17g,\"perimeter\":%lld,\"solidity\":%.17g,\"obb\":[[%.17g,%.17g],[%.17g,%.17g],[%.17g,%.17g],[%.17g,%.17g]]",
                    p->cx, p->cy, p->orientation, p->perimeter, p->solidity, p->obb[0], p->obb[1], p->obb[2], p->obb[3], p->obb[4], p->obb[5], p->obb[6], p->obb[7]);
        }
        fprintf(g, "}}");
    }
    fprintf(g, "\n]}\n");
}

int main(int argc, char** argv)
{
    const int host = argc > 1 && strcmp(argv[1], "--host") == 0;
    const int simplify = argc > 1 + host && strcmp(argv[1 + host], "--tolerance") == 0;
    const int geo = argc > 1 + host + 2 * simplify && strcmp(argv[1 + host + 2 * simplify], "--geojson") == 0;
    const int geo_at = 1 + host + 2 * simplify;
    int small = 0, fill = 0, disjoint = 0, props = 0, area_at = 0, file = geo_at + 2 * geo;
    for (int turn = 0; turn < 4; ++turn) {                       /* the two component flags, --disjoint and --props, in any order, once each */
        if (!small && argc > file + 1 && strcmp(argv[file], "--min-area") == 0) { small = 1; area_at = file + 1; file += 2; }
        else if (!fill && argc > file && strcmp(argv[file], "--fill-holes") == 0) { fill = 1; file += 1; }
        else if (!disjoint && argc > file && strcmp(argv[file], "--disjoint") == 0) { disjoint = 1; file += 1; }
        else if (!props && argc > file && strcmp(argv[file], "--props") == 0) { props = 1; file += 1; }
    }
    if (argc != file + 1 || strncmp(argv[file], "--", 2) == 0) {         /* (a flag out of place, or one without its value) */
        fprintf(stderr, "usage: %s [--host] [--tolerance T] [--geojson FILE] [--props] [--min-area A] [--fill-holes] [--disjoint] <set.txt>\n", argv[0]);
        return 64;
    }
    const double tolerance = simplify ? atof(argv[2 + host]) : 0.0;
    const long long min_area = small ? atoll(argv[area_at]) : 0;
    const char* geo_file = geo ? argv[geo_at + 1] : NULL;
    FILE* f = fopen(argv[file], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[file]); return 66; }
    int n_images = 0, slots = 0;
    if (fscanf(f, "%d %d", &n_images, &slots) != 2 || n_images < 0 || slots < 0 || (n_images > 0 && slots > 1000000 / n_images)) {
        fprintf(stderr, "%s: n_images and slots expected\n", argv[file]);
        return 65;
    }
    const size_t n = (size_t)n_images * (size_t)slots;
    int32_t* heights = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_images + 1));
    int32_t* widths = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_images + 1));
    int64_t* run_offsets = (int64_t*)malloc(sizeof(int64_t) * (n + 1));
    int64_t* rle_rings = (int64_t*)malloc(sizeof(int64_t) * (n + 1));
    size_t held = 1024, used = 0;
    uint32_t* counts = (uint32_t*)malloc(sizeof(uint32_t) * held);
    if (!heights || !widths || !run_offsets || !rle_rings || !counts) { fprintf(stderr, "out of memory\n"); return 70; }
    run_offsets[0] = 0;
    for (int b = 0; b < n_images; ++b) {
        if (fscanf(f, "%d %d", &heights[b], &widths[b]) != 2) { fprintf(stderr, "image %d: height and width expected\n", b); return 65; }
        for (int i = 0; i < slots; ++i) {
            long long runs = 0;
            if (fscanf(f, "%lld", &runs) != 1 || runs < 0 || runs > 0x7fffffffLL) { fprintf(stderr, "image %d, RLE %d: the number of runs expected\n", b, i); return 65; }
            if (used + (size_t)runs > held) {
                while (used + (size_t)runs > held) held *= 2;
                counts = (uint32_t*)realloc(counts, sizeof(uint32_t) * held);
                if (!counts) { fprintf(stderr, "out of memory\n"); return 70; }
            }
            for (long long j = 0; j < runs; ++j) {
                unsigned long c = 0;
                if (fscanf(f, "%lu", &c) != 1) { fprintf(stderr, "image %d, RLE %d: %lld runs expected\n", b, i, runs); return 65; }
                counts[used++] = (uint32_t)c;
            }
            run_offsets[(size_t)b * (size_t)slots + (size_t)i + 1] = (int64_t)used;
        }
    }
    fclose(f);

    mask_props* shape = NULL;
    if (fill || small || disjoint || props) {                    /* per RLE sizes; holes first, then specks, then the overlaps, then the measures */
        int32_t* hs = (int32_t*)malloc(sizeof(int32_t) * (n + 1));
        int32_t* ws = (int32_t*)malloc(sizeof(int32_t) * (n + 1));
        if (!hs || !ws) { fprintf(stderr, "out of memory\n"); return 70; }
        for (size_t k = 0; k < n; ++k) { hs[k] = heights[k / (size_t)slots]; ws[k] = widths[k / (size_t)slots]; }
        int st = fill ? filter_components(host, MRCNN_COMPONENTS_OF_ZEROS, &counts, run_offsets, (int64_t)n, hs, ws, 0) : MRCNN_OK;
        if (st == MRCNN_OK && small) st = filter_components(host, MRCNN_COMPONENTS_OF_ONES, &counts, run_offsets, (int64_t)n, hs, ws, min_area);
        if (st == -1) { fprintf(stderr, "out of memory\n"); return 70; }
        if (st != MRCNN_OK) {
            fprintf(stderr, "mrcnn_rle_components%s failed (%d): %s\n", host ? "_host" : "", st, mrcnn_last_error());
            return st;
        }
        if (disjoint) st = make_disjoint(host, &counts, run_offsets, n_images, slots, hs, ws);
        if (st == -1) { fprintf(stderr, "out of memory\n"); return 70; }
        if (st != MRCNN_OK) {
            fprintf(stderr, "mrcnn_rle_combine%s failed (%d): %s\n", host ? "_host" : "", st, mrcnn_last_error());
            return st;
        }
        if (props) {
            shape = (mask_props*)malloc(sizeof(mask_props) * (n + 1));
            st = shape ? measure_props(host, counts, run_offsets, (int64_t)n, hs, ws, shape) : -1;
            if (st == -1) { fprintf(stderr, "out of memory\n"); return 70; }
            if (st != MRCNN_OK) {
                fprintf(stderr, "measuring the masks failed (%d): %s\n", st, mrcnn_last_error());
                return st;
            }
        }
        free(ws); free(hs);
    }

    /* the size query: no buffers, both capacities 0.  MRCNN_ERR_SHAPE is its answer when there is anything to write. */
    int64_t rings = 0, vertices = 0;
    int st = trace(host, counts, run_offsets, n_images, slots, heights, widths, rle_rings, &rings, &vertices, NULL, NULL, 0, NULL, 0);
    if (st != MRCNN_OK && !(st == MRCNN_ERR_SHAPE && (rings > 0 || vertices > 0))) {
        fprintf(stderr, "the size query failed (%d): %s\n", st, mrcnn_last_error());
        return st;
    }
    int64_t* ring_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
    int64_t* ring_areas = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
    int32_t* xy = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(vertices + 1));
    if (!ring_offsets || !ring_areas || !xy) { fprintf(stderr, "out of memory\n"); return 70; }
    st = trace(host, counts, run_offsets, n_images, slots, heights, widths, rle_rings, &rings, &vertices, ring_offsets, ring_areas, rings, xy, vertices);
    if (st != MRCNN_OK) {
        fprintf(stderr, "mrcnn_rle_to_polygons%s failed (%d): %s\n", host ? "_host" : "", st, mrcnn_last_error());
        return st;
    }
    int64_t *rle_polys = NULL, *poly_rings = NULL, *ring_order = NULL;
    if (geo) {
        /* nested where the rings are still the traced ones: simplification keeps them one for one, so the nesting indexes the simplified
         * rings too.  n_polys <= rings: the buffers are sized by the rings, no size query. */
        int64_t* parent = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
        int32_t* depth = (int32_t*)malloc(sizeof(int32_t) * (size_t)(rings + 1));
        int64_t polys = 0;
        rle_polys = (int64_t*)malloc(sizeof(int64_t) * (n + 1));
        poly_rings = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
        ring_order = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
        if (!parent || !depth || !rle_polys || !poly_rings || !ring_order) { fprintf(stderr, "out of memory\n"); return 70; }
        st = host ? mrcnn_polygons_nest_host(rle_rings, (int64_t)n, ring_offsets, xy, rings, parent, depth, rle_polys, poly_rings, ring_order, &polys)
                  : mrcnn_polygons_nest(rle_rings, (int64_t)n, ring_offsets, xy, rings, MRCNN_HOST, parent, depth, rle_polys, poly_rings, ring_order, &polys);
        if (st != MRCNN_OK) {
            fprintf(stderr, "mrcnn_polygons_nest%s failed (%d): %s\n", host ? "_host" : "", st, mrcnn_last_error());
            return st;
        }
        free(depth); free(parent);
    }
    if (simplify) {
        /* the input's vertex count always suffices as the capacity: no size query.  The rings stay in their order, so rle_rings and the
         * pixel areas still go with them. */
        int64_t* simple_offsets = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rings + 1));
        int32_t* simple_xy = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(vertices + 1));
        int64_t simple_vertices = 0;
        if (!simple_offsets || !simple_xy) { fprintf(stderr, "out of memory\n"); return 70; }
        st = host ? mrcnn_polygons_simplify_host(ring_offsets, xy, rings, tolerance, simple_offsets, NULL, simple_xy, NULL, &simple_vertices, vertices)
                  : mrcnn_polygons_simplify(ring_offsets, xy, rings, tolerance, MRCNN_HOST, simple_offsets, NULL, simple_xy, NULL, &simple_vertices, vertices);
        if (st != MRCNN_OK) {
            fprintf(stderr, "mrcnn_polygons_simplify%s failed (%d): %s\n", host ? "_host" : "", st, mrcnn_last_error());
            return st;
        }
        printf("%lld rings, %lld vertices, %lld simplified within %g px, in %d x %d RLEs\n", (long long)rings, (long long)vertices,
               (long long)simple_vertices, tolerance, n_images, slots);
        free(xy); free(ring_offsets);
        xy = simple_xy; ring_offsets = simple_offsets;
    } else
        printf("%lld rings, %lld vertices in %d x %d RLEs\n", (long long)rings, (long long)vertices, n_images, slots);
    for (size_t k = 0; k < n; ++k)
        for (int64_t r = rle_rings[k]; r < rle_rings[k + 1]; ++r) {
            printf("RLE %lld ring %lld area %lld:", (long long)k, (long long)(r - rle_rings[k]), (long long)ring_areas[r]);
            for (int64_t v = ring_offsets[r]; v < ring_offsets[r + 1]; ++v) printf(" %d,%d", (int)xy[2 * v], (int)xy[2 * v + 1]);
            printf("\n");
        }
    for (size_t k = 0; shape && k < n; ++k) {
        const mask_props* p = shape + k;
        if (!p->any) continue;
        printf("RLE %lld props: area %lld perimeter %lld centroid %.17g %.17g orientation %.17g solidity %.17g obb %.17g,%.17g %.17g,%.17g %.17g,%.17g %.17g,%.17g\n",
               (long long)k, p->area, p->perimeter, p->cx, p->cy, p->orientation, p->solidity, p->obb[0], p->obb[1], p->obb[2], p->obb[3], p->obb[4], p->obb[5],
               p->obb[6], p->obb[7]);
    }
    if (geo) {
        FILE* g = fopen(geo_file, "w");
        if (!g) { fprintf(stderr, "cannot write %s\n", geo_file); return 73; }
        write_geojson(g, n, slots, rle_rings, ring_offsets, ring_areas, xy, rle_polys, poly_rings, ring_order, shape);
        if (fclose(g) != 0) { fprintf(stderr, "cannot write %s\n", geo_file); return 74; }
        free(ring_order); free(poly_rings); free(rle_polys);
    }
    free(shape); free(xy); free(ring_areas); free(ring_offsets); free(counts); free(rle_rings); free(run_offsets); free(widths); free(heights);
    return 0;
}
