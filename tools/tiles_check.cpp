// tiles_check.cpp — the host half of tiled prediction (csrc/tiles_host.cpp: the planner and the definitions of the merge and of the
// union) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc
//       tools/tiles_check.cpp mask-rcnn-coreml_amd/csrc/tiles_host.cpp -o tiles_check            (one command line)
//   ./tiles_check
//
// Host code only: no GPU, no HIP, no Python.  Seeded scenes — one or two images of 1x1 .. 90x90, random windows (some equal, some a
// single pixel, some the whole image), 1..5 rows a tile, masks of 2x2 .. 28x28 of noise, boxes anywhere including the borders — go
// through the planner and through the merge three times: the size query, a counts buffer one run short, and a buffer of exactly the
// size reported.  Every output lives in a heap block of exactly its documented size, so a write past any of them is a report.  The
// results are then checked for what must hold whatever the scene: every RLE sums to its image's pixels with no empty run behind the
// first, the areas are the sums of the odd runs, kept candidates are distinct, eligible, of the right image and in score order, padding
// is -1 / zero rows / the single run [h*w].  The same scenes then go through the union (unite_host) with the same three calls and
// exact-size blocks, n_parts and group included: the RLEs sum to the image's pixels with no empty run behind the first, the areas are
// the sums of the odd runs, the parts of the components add up to the eligible candidates when nothing is truncated, and group agrees
// with source and n_parts.  Exit status: 0 = clean; 1 = a finding; a sanitizer report ends the program with the
// sanitizer's own non-zero status.
#include <math.h>
#include <stdio.h>

#include <random>
#include <set>
#include <string>
#include <vector>

#include "tiles_host.h"

// the library's arithmetic (api.hip), restated: this program links nothing but tiles_host.cpp
extern "C" int mrcnn_letterbox_geometry(int h, int w, int H, int W, int* nh, int* nw, int* pad_y, int* pad_x)
{
    const double sc = fmin((double)W / (double)w, (double)H / (double)h);
    int a = (int)floor((double)h * sc + 0.5), b = (int)floor((double)w * sc + 0.5);
    a = a < 1 ? 1 : (a > H ? H : a);
    b = b < 1 ? 1 : (b > W ? W : b);
    *nh = a; *nw = b; *pad_y = (H - a) / 2; *pad_x = (W - b) / 2;
    return MRCNN_OK;
}

using namespace mrcnn;

#define FINDING(...) do { fprintf(stderr, "seed %u: ", seed); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static int one(unsigned seed)
{
    std::mt19937 rng(seed);
    auto U = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto F = [&] { return (float)(rng() % 10001) / 10000.0f; };
    const int B = U(1, 2), rows = U(1, 5), S = U(0, 3) == 0 ? U(2, 6) : 28, model = U(0, 1) ? 64 : 128, max_out = U(1, 7);
    std::vector<int32_t> hs((size_t)B), ws((size_t)B);
    for (int b = 0; b < B; ++b) { hs[(size_t)b] = U(1, 90); ws[(size_t)b] = U(1, 90); }
    // the planner on image 0, with exact-size storage
    std::string err;
    {
        const int th = U(1, 100), tw = U(1, 100), oy = U(0, th - 1), ox = U(0, tw - 1);
        int n = -1;
        if (tiles::plan(hs[0], ws[0], th, tw, oy, ox, 0, nullptr, 0, &n, &err) != MRCNN_OK || n < 1) FINDING("plan: size query failed");
        std::vector<mrcnn_tile> out((size_t)n);
        if (n > 1 && tiles::plan(hs[0], ws[0], th, tw, oy, ox, 0, out.data(), n - 1, &n, &err) != MRCNN_ERR_SHAPE) FINDING("plan: a short table was accepted");
        if (tiles::plan(hs[0], ws[0], th, tw, oy, ox, 0, out.data(), n, &n, &err) != MRCNN_OK) FINDING("plan failed: %s", err.c_str());
        if (tiles::check_tiles(out.data(), n, hs.data(), ws.data(), B, "check", &err) != MRCNN_OK) FINDING("plan: %s", err.c_str());
    }
    const int T = U(1, 6);
    std::vector<mrcnn_tile> tl((size_t)T);
    for (int t = 0; t < T; ++t) {
        mrcnn_tile& w = tl[(size_t)t];
        if (t > 0 && U(0, 3) == 0) { w = tl[(size_t)t - 1]; continue; }           // the same window again
        w.image = U(0, B - 1);
        const int h = hs[(size_t)w.image], wd = ws[(size_t)w.image];
        w.height = U(0, 4) == 0 ? h : U(1, h); w.width = U(0, 4) == 0 ? wd : U(1, wd);
        w.y0 = U(0, h - w.height); w.x0 = U(0, wd - w.width);
    }
    const size_t n = (size_t)T * rows, slots = (size_t)B * max_out;
    std::vector<float> det(n * 6), masks(n * S * S);
    for (size_t k = 0; k < n; ++k) {
        float* d = &det[k * 6];
        const float y1 = F(), x1 = F();
        d[0] = y1; d[1] = x1; d[2] = U(0, 5) == 0 ? 1.0f : y1 + (1.0f - y1) * F(); d[3] = U(0, 5) == 0 ? 1.0f : x1 + (1.0f - x1) * F();
        d[4] = (float)U(1, 2); d[5] = U(0, 6) == 0 ? 0.0f : (float)U(1, 4) / 4.0f;           // few score values: ties
        if (U(0, 7) == 0) d[0] = d[1] = d[2] = d[3] = 0.0f;                                 // a padding row
    }
    for (float& v : masks) v = F();
    std::vector<float> src(slots * 6);
    std::vector<int32_t> source(slots), n_kept((size_t)B), boxes(slots * 4);
    std::vector<int64_t> ro(slots + 1);
    std::vector<uint32_t> areas(slots);
    tiles::MergeArgs a{det.data(), masks.data(), tl.data(), T, rows, S, hs.data(), ws.data(), B, model, model, 0.5f, U(0, 1), U(0, 1) ? 0.5 : 0.0625 * U(1, 16),
                       max_out, src.data(), source.data(), n_kept.data(), nullptr, 0, ro.data(), areas.data(), boxes.data()};
    if (tiles::merge_host(a, &err) != MRCNN_ERR_SHAPE) FINDING("the size query did not answer MRCNN_ERR_SHAPE");
    const int64_t need = ro[slots];
    if (need < (int64_t)slots) FINDING("fewer runs than slots");
    std::vector<uint32_t> shorter((size_t)need - 1), counts((size_t)need);
    a.counts = shorter.data(); a.capacity = need - 1;
    if (tiles::merge_host(a, &err) != MRCNN_ERR_SHAPE) FINDING("a short counts buffer was accepted");
    a.counts = counts.data(); a.capacity = need;
    if (tiles::merge_host(a, &err) != MRCNN_OK) FINDING("merge failed: %s", err.c_str());
    if (ro[slots] != need) FINDING("the size changed between calls");
    std::set<int32_t> seen;
    for (int b = 0; b < B; ++b) {
        const uint64_t pixels = (uint64_t)hs[(size_t)b] * (uint64_t)ws[(size_t)b];
        float last = INFINITY;
        int filled = 0;
        for (int j = 0; j < max_out; ++j) {
            const size_t s = (size_t)b * max_out + j;
            const int64_t r0 = ro[s], r1 = ro[s + 1];
            uint64_t sum = 0, ones = 0;
            for (int64_t i = r0; i < r1; ++i) {
                sum += counts[(size_t)i];
                if ((i - r0) & 1) ones += counts[(size_t)i];
                if (i > r0 && counts[(size_t)i] == 0) FINDING("an empty run behind the first");
            }
            if (r1 <= r0 || sum != pixels || ones != areas[s]) FINDING("slot %zu: runs sum to %llu of %llu, area %u against %llu", s, (unsigned long long)sum,
                                                                     (unsigned long long)pixels, areas[s], (unsigned long long)ones);
            const int32_t k = source[s];
            if (k < 0) {
                if (k != -1 || r1 - r0 != 1 || areas[s] != 0 || src[s * 6 + 5] != 0.0f) FINDING("slot %zu: bad padding", s);
                continue;
            }
            if (j != filled++) FINDING("slot %zu: a kept row behind padding", s);
            if ((size_t)k >= n || tl[(size_t)k / rows].image != b || !(det[(size_t)k * 6 + 5] > 0.0f) || !seen.insert(k).second) FINDING("slot %zu: bad source %d", s, k);
            if (src[s * 6 + 5] != det[(size_t)k * 6 + 5] || src[s * 6 + 4] != det[(size_t)k * 6 + 4] || src[s * 6 + 5] > last) FINDING("slot %zu: bad row or order", s);
            last = src[s * 6 + 5];
            if (!(src[s * 6] >= 0.0f && src[s * 6 + 2] <= 1.0f && src[s * 6] <= src[s * 6 + 2] && src[s * 6 + 1] <= src[s * 6 + 3] && src[s * 6 + 3] <= 1.0f)) FINDING("slot %zu: bad box", s);
        }
        if (n_kept[(size_t)b] < filled || (n_kept[(size_t)b] > filled && filled != max_out)) FINDING("image %d: n_kept %d against %d rows", b, n_kept[(size_t)b], filled);
    }
    return 0;
}

static long g_united = 0;                   // components of more than one member, over all scenes: the check has teeth only if there are some

// the same scene through the union
static int two(unsigned seed)
{
    std::mt19937 rng(seed);
    auto U = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto F = [&] { return (float)(rng() % 10001) / 10000.0f; };
    const int B = U(1, 2), rows = U(1, 5), S = U(0, 3) == 0 ? U(2, 6) : 28, model = U(0, 1) ? 64 : 128, max_out = U(1, 7);
    std::vector<int32_t> hs((size_t)B), ws((size_t)B);
    for (int b = 0; b < B; ++b) { hs[(size_t)b] = U(1, 90); ws[(size_t)b] = U(1, 90); }
    const int T = U(1, 6);
    std::vector<mrcnn_tile> tl((size_t)T);
    for (int t = 0; t < T; ++t) {
        mrcnn_tile& w = tl[(size_t)t];
        if (t > 0 && U(0, 3) == 0) { w = tl[(size_t)t - 1]; continue; }
        w.image = U(0, B - 1);
        const int h = hs[(size_t)w.image], wd = ws[(size_t)w.image];
        w.height = U(0, 4) == 0 ? h : U(1, h); w.width = U(0, 4) == 0 ? wd : U(1, wd);
        w.y0 = U(0, h - w.height); w.x0 = U(0, wd - w.width);
    }
    const size_t n = (size_t)T * rows, slots = (size_t)B * max_out;
    std::vector<float> det(n * 6), masks(n * S * S);
    for (size_t k = 0; k < n; ++k) {
        float* d = &det[k * 6];
        const float y1 = F(), x1 = F();
        d[0] = y1; d[1] = x1; d[2] = U(0, 5) == 0 ? 1.0f : y1 + (1.0f - y1) * F(); d[3] = U(0, 5) == 0 ? 1.0f : x1 + (1.0f - x1) * F();
        d[4] = (float)U(1, 2); d[5] = U(0, 6) == 0 ? 0.0f : (float)U(1, 4) / 4.0f;
        if (U(0, 7) == 0) d[0] = d[1] = d[2] = d[3] = 0.0f;
    }
    for (float& v : masks) v = U(0, 2) == 0 ? 0.9f : F();                                   // a third of the cells set: planes that meet
    std::vector<float> src(slots * 6);
    std::vector<int32_t> source(slots), n_kept((size_t)B), boxes(slots * 4), n_parts(slots), group(n);
    std::vector<int64_t> ro(slots + 1);
    std::vector<uint32_t> areas(slots);
    std::string err;
    tiles::MergeArgs a{det.data(), masks.data(), tl.data(), T, rows, S, hs.data(), ws.data(), B, model, model, 0.5f, U(0, 1), 0.0625 * U(1, 16),
                       max_out, src.data(), source.data(), n_kept.data(), nullptr, 0, ro.data(), areas.data(), boxes.data(), n_parts.data(), group.data()};
    if (tiles::unite_host(a, &err) != MRCNN_ERR_SHAPE) FINDING("unite: the size query did not answer MRCNN_ERR_SHAPE");
    const int64_t need = ro[slots];
    if (need < (int64_t)slots) FINDING("unite: fewer runs than slots");
    std::vector<uint32_t> shorter((size_t)need - 1), counts((size_t)need);
    a.counts = shorter.data(); a.capacity = need - 1;
    if (tiles::unite_host(a, &err) != MRCNN_ERR_SHAPE) FINDING("unite: a short counts buffer was accepted");
    a.counts = counts.data(); a.capacity = need;
    a.n_parts = nullptr; a.group = nullptr;                                                  // both may be null
    if (tiles::unite_host(a, &err) != MRCNN_OK) FINDING("unite failed: %s", err.c_str());
    a.n_parts = n_parts.data(); a.group = group.data();
    if (tiles::unite_host(a, &err) != MRCNN_OK) FINDING("unite failed: %s", err.c_str());
    if (ro[slots] != need) FINDING("unite: the size changed between calls");
    for (int b = 0; b < B; ++b) {
        const uint64_t pixels = (uint64_t)hs[(size_t)b] * (uint64_t)ws[(size_t)b];
        long parts = 0, in_groups = 0;
        int filled = 0;
        float last = INFINITY;
        for (int j = 0; j < max_out; ++j) {
            const size_t s = (size_t)b * max_out + j;
            const int64_t r0 = ro[s], r1 = ro[s + 1];
            uint64_t sum = 0, ones = 0;
            for (int64_t i = r0; i < r1; ++i) {
                sum += counts[(size_t)i];
                if ((i - r0) & 1) ones += counts[(size_t)i];
                if (i > r0 && counts[(size_t)i] == 0) FINDING("unite: an empty run behind the first");
            }
            if (r1 <= r0 || sum != pixels || ones != areas[s]) FINDING("unite slot %zu: runs sum to %llu of %llu, area %u against %llu", s, (unsigned long long)sum,
                                                                     (unsigned long long)pixels, areas[s], (unsigned long long)ones);
            const int32_t k = source[s];
            if (k < 0) {
                if (k != -1 || r1 - r0 != 1 || areas[s] != 0 || n_parts[s] != 0 || src[s * 6 + 5] != 0.0f) FINDING("unite slot %zu: bad padding", s);
                continue;
            }
            if (j != filled++) FINDING("unite slot %zu: a component behind padding", s);
            if ((size_t)k >= n || tl[(size_t)k / rows].image != b || group[(size_t)k] != j) FINDING("unite slot %zu: source %d is not of group %d", s, k, j);
            if (src[s * 6 + 5] != det[(size_t)k * 6 + 5] || src[s * 6 + 4] != det[(size_t)k * 6 + 4] || src[s * 6 + 5] > last) FINDING("unite slot %zu: bad row or order", s);
            last = src[s * 6 + 5];
            long members = 0;
            for (size_t c = 0; c < n; ++c)
                if (tl[c / rows].image == b && group[c] == j) {
                    ++members;
                    if (det[c * 6 + 4] != det[(size_t)k * 6 + 4] || det[c * 6 + 5] > det[(size_t)k * 6 + 5] || (det[c * 6 + 5] == det[(size_t)k * 6 + 5] && (int32_t)c < k))
                        FINDING("unite slot %zu: member %zu against representative %d", s, c, k);
                }
            if (members != n_parts[s] || members < 1) FINDING("unite slot %zu: n_parts %d against %ld members", s, n_parts[s], members);
            parts += members;
            if (members > 1) ++g_united;
        }
        int32_t top = -1;
        for (size_t c = 0; c < n; ++c)
            if (tl[c / rows].image == b && group[c] >= 0) { ++in_groups; top = group[c] > top ? group[c] : top; }
        if (top + 1 != n_kept[(size_t)b]) FINDING("unite image %d: n_kept %d against the highest group %d", b, n_kept[(size_t)b], top);
        if (n_kept[(size_t)b] <= max_out && parts != in_groups) FINDING("unite image %d: %ld parts against %ld eligible candidates", b, parts, in_groups);
        if (n_kept[(size_t)b] < filled || (n_kept[(size_t)b] > filled && filled != max_out)) FINDING("unite image %d: n_kept %d against %d slots", b, n_kept[(size_t)b], filled);
    }
    for (size_t c = 0; c < n; ++c)
        if (group[c] < -1 || (!(det[c * 6 + 5] > 0.0f) && group[c] != -1)) FINDING("unite: candidate %zu without a score has group %d", c, group[c]);
    return 0;
}

int main()
{
    for (unsigned seed = 1; seed <= 4000; ++seed)
        if (one(seed) || two(seed)) return 1;
    if (g_united < 1000) { fprintf(stderr, "only %ld united components in 4000 scenes\n", g_united); return 1; }
    printf("tiles_check: 4000 scenes clean through the merge and through the union (%ld components of several parts)\n", g_united);
    return 0;
}
