// rle_draw_check.cpp — the host definitions of the RLE drawing entries (csrc/rle_draw_host.cpp) under the sanitizers, as a program of
// its own:
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc
//       tools/rle_draw_check.cpp mask-rcnn-coreml_amd/csrc/rle_draw_host.cpp mask-rcnn-coreml_amd/csrc/rle_set_host.cpp -o rle_draw_check
//                                                                                                    (one command line)
//   ./rle_draw_check
//
// Host code only: no GPU, no HIP, no Python.  Seeded scenes — one to three images of 1x1 .. 40x40, 0..5 slots, planes of noise encoded
// with zero-length runs thrown in, rows anywhere including boxes outside the image, NaN and huge coordinates — go through the decode,
// the map and the overlay.  Every output lives in a heap block of exactly its documented extent, with a 16- or 48-byte gap before
// every image, so a write past any of them is a report; the gaps must keep their fill.  The results are compared with dense planes
// painted here pixel by pixel.  Then one count of one RLE is moved by one: every entry must answer MRCNN_ERR_SHAPE, name the RLE and
// leave its outputs as they were.  Exit status: 0 = clean; 1 = a finding; a sanitizer report ends the program with the sanitizer's
// own non-zero status.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "draw_rule.h"
#include "rle_draw_host.h"

using namespace mrcnn;

static int findings = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("scene %d: ", scene);                    \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
            if (++findings > 20) return 1;                  \
        }                                                   \
    } while (0)

int main()
{
    std::mt19937 rng(20261019);
    auto uni = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    for (int scene = 0; scene < 3000; ++scene) {
        const int B = uni(1, 3), slots = uni(0, 5), n = B * slots;
        std::vector<int32_t> hs((size_t)B), ws((size_t)B);
        for (int b = 0; b < B; ++b) { hs[(size_t)b] = uni(1, scene % 7 ? 12 : 40); ws[(size_t)b] = uni(1, scene % 5 ? 12 : 40); }
        // planes, their runs (with empty runs thrown in) and the rows
        std::vector<std::vector<uint8_t>> planes((size_t)n);
        std::vector<uint32_t> counts;
        std::vector<int64_t> offs{0};
        std::vector<float> det((size_t)n * 6 + 1, 0.0f);
        for (int k = 0; k < n; ++k) {
            const int h = hs[(size_t)(k / slots)], w = ws[(size_t)(k / slots)], density = uni(0, 4);
            auto& p = planes[(size_t)k];
            p.assign((size_t)h * w, 0);
            for (auto& v : p) v = density == 0 ? 0 : (density == 4 ? 1 : (uint8_t)(uni(0, 3) < density));
            uint8_t cur = 0;
            uint32_t run = 0;
            for (int q = 0; q < h * w; ++q) {                                // column-major: q = x*h + y
                const uint8_t v = p[(size_t)(q % h) * w + q / h];
                const bool split = uni(0, 15) == 0;                          // an empty run of the other value inside a run
                if (v != cur || split) {
                    counts.push_back(run); run = 0;
                    if (v == cur) counts.push_back(0); else cur = v;
                }
                ++run;
            }
            counts.push_back(run);
            if (uni(0, 3) == 0) counts.push_back(0);                         // a trailing empty run
            offs.push_back((int64_t)counts.size());
            float* r = &det[(size_t)k * 6];
            const float y1 = (float)uni(-2, 10) / 10.0f, x1 = (float)uni(-2, 10) / 10.0f;
            r[0] = y1; r[1] = x1; r[2] = y1 + (float)uni(-1, 8) / 10.0f; r[3] = x1 + (float)uni(-1, 8) / 10.0f; r[4] = 1.0f;
            r[5] = uni(0, 4) == 0 ? 0.0f : (float)uni(1, 99) / 100.0f;
            if (uni(0, 40) == 0) r[uni(0, 3)] = NAN;
            if (uni(0, 40) == 0) r[uni(0, 3)] = 3e30f;
        }
        if (counts.empty()) counts.push_back(0);
        const float min_score = (float)uni(0, 60) / 100.0f;
        const int alpha = uni(0, 256), stroke = uni(0, 5), grow = stroke / 2, shrink = stroke - stroke / 2;
        const rle_draw::Set set{counts.data(), offs.data(), B, slots, hs.data(), ws.data()};
        // ragged layouts with a gap before every image, the buffers exactly as long as the last image's end
        auto layout = [&](int64_t unit_of_image(int, const void*), const void* ctx, std::vector<int64_t>& at) {
            int64_t o = 0;
            at.assign((size_t)B, 0);
            int64_t end = 0;
            for (int b = 0; b < B; ++b) {
                o = (o + 15) / 16 * 16 + (scene & 1 ? 16 : 48);
                at[(size_t)b] = o;
                o += unit_of_image(b, ctx);
                end = o;
            }
            return end;
        };
        struct Ctx { const int32_t* hs; const int32_t* ws; int slots; } ctx{hs.data(), ws.data(), slots};
        std::vector<int64_t> o_dec, o_map, o_rgb;
        const int64_t n_dec = layout([](int b, const void* c) { auto* x = (const Ctx*)c; return (int64_t)x->slots * x->hs[b] * x->ws[b]; }, &ctx, o_dec);
        const int64_t n_map = layout([](int b, const void* c) { auto* x = (const Ctx*)c; return (int64_t)2 * x->hs[b] * x->ws[b]; }, &ctx, o_map);
        const int64_t n_rgb = layout([](int b, const void* c) { auto* x = (const Ctx*)c; return (int64_t)3 * x->hs[b] * x->ws[b]; }, &ctx, o_rgb);
        std::vector<uint8_t> dec((size_t)n_dec, 0x5a), rgb((size_t)n_rgb, 0x5a);
        std::vector<int16_t> map((size_t)(n_map + 1) / 2, 0x5a5a);
        std::vector<uint32_t> vis((size_t)n, 77u);
        std::vector<std::vector<uint8_t>> src((size_t)B);
        std::vector<mrcnn_image> images((size_t)B);
        for (int b = 0; b < B; ++b) {
            src[(size_t)b].resize((size_t)3 * hs[(size_t)b] * ws[(size_t)b]);
            for (auto& v : src[(size_t)b]) v = (uint8_t)uni(0, 255);
            images[(size_t)b] = mrcnn_image{src[(size_t)b].data(), hs[(size_t)b], ws[(size_t)b]};
        }
        std::string err;
        int st = rle_draw::decode_host(set, dec.data(), o_dec.data(), &err);
        EXPECT(st == MRCNN_OK, "decode: %d %s", st, err.c_str());
        st = rle_draw::instance_map_host(set, det.data(), min_score, map.data(), o_map.data(), n ? vis.data() : nullptr, &err);
        EXPECT(st == MRCNN_OK, "map: %d %s", st, err.c_str());
        st = rle_draw::render_host(set, images.data(), det.data(), min_score, alpha, stroke, rgb.data(), o_rgb.data(), &err);
        EXPECT(st == MRCNN_OK, "render: %d %s", st, err.c_str());
        // the same from dense planes, pixel by pixel
        std::vector<uint8_t> w_dec((size_t)n_dec, 0x5a), w_rgb((size_t)n_rgb, 0x5a);
        std::vector<int16_t> w_map((size_t)(n_map + 1) / 2, 0x5a5a);
        for (int b = 0; b < B; ++b) {
            const int h = hs[(size_t)b], w = ws[(size_t)b];
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    int own = -1, ring = -1;
                    for (int i = 0; i < slots; ++i) {
                        const int k = b * slots + i;
                        w_dec[(size_t)(o_dec[(size_t)b] + ((int64_t)i * h + y) * w + x)] = planes[(size_t)k][(size_t)y * w + x];
                        const float* r = &det[(size_t)k * 6];
                        const RleDrawBox bx = rle_draw_box(r, h, w);
                        if (!(r[5] > min_score && r[5] > 0.0f && bx.y2 > bx.y1 && bx.x2 > bx.x1)) continue;
                        if (own < 0 && planes[(size_t)k][(size_t)y * w + x]) own = i;
                        if (ring < 0 && stroke > 0 && in_ring(bx, grow, shrink, y, x)) ring = i;
                    }
                    reinterpret_cast<int16_t*>(reinterpret_cast<uint8_t*>(w_map.data()) + o_map[(size_t)b])[(size_t)y * w + x] = (int16_t)own;
                    static const int pal[4][3] = {{255, 0, 0}, {0, 0, 255}, {0, 255, 0}, {255, 255, 0}};
                    for (int c = 0; c < 3; ++c) {
                        const int s = src[(size_t)b][((size_t)y * w + x) * 3 + c];
                        const int v = ring >= 0 ? pal[ring % 4][c] : (own >= 0 ? (s * (256 - alpha) + pal[own % 4][c] * alpha + 128) >> 8 : s);
                        w_rgb[(size_t)(o_rgb[(size_t)b] + ((int64_t)y * w + x) * 3 + c)] = (uint8_t)v;
                    }
                }
        }
        EXPECT(dec == w_dec, "the planes differ (or a gap was written)");
        EXPECT(memcmp(map.data(), w_map.data(), (size_t)n_map) == 0, "the map differs (or a gap was written)");
        EXPECT(rgb == w_rgb, "the overlay differs (or a gap was written)");
        for (int k = 0; k < n; ++k) {
            const int b = k / slots, i = k % slots;
            uint32_t want = 0;
            const int16_t* m = reinterpret_cast<const int16_t*>(reinterpret_cast<const uint8_t*>(w_map.data()) + o_map[(size_t)b]);
            for (int q = 0; q < hs[(size_t)b] * ws[(size_t)b]; ++q) want += m[q] == i;
            EXPECT(vis[(size_t)k] == want, "visible[%d] = %u, %u pixels are its own", k, vis[(size_t)k], want);
        }
        // one count moved by one: refused, named, nothing written
        if (n > 0) {
            const int k = uni(0, n - 1);
            std::vector<uint32_t> bad = counts;
            int64_t j = offs[(size_t)k];
            const bool up = uni(0, 1) == 1;
            if (!up) while (bad[(size_t)j] == 0) ++j;                         // (a run that has a pixel to give: the plane has h*w >= 1)
            bad[(size_t)j] += up ? 1u : 0xffffffffu;
            const rle_draw::Set bset{bad.data(), offs.data(), B, slots, hs.data(), ws.data()};
            const std::vector<uint8_t> dec0 = dec, rgb0 = rgb;
            const std::vector<int16_t> map0 = map;
            const std::vector<uint32_t> vis0 = vis;
            const std::string name = "RLE " + std::to_string(k) + " ";
            st = rle_draw::decode_host(bset, dec.data(), o_dec.data(), &err);
            EXPECT(st == MRCNN_ERR_SHAPE && err.find(name) != std::string::npos && dec == dec0, "decode of a bad RLE: %d %s", st, err.c_str());
            st = rle_draw::instance_map_host(bset, det.data(), min_score, map.data(), o_map.data(), vis.data(), &err);
            EXPECT(st == MRCNN_ERR_SHAPE && err.find(name) != std::string::npos && map == map0 && vis == vis0, "map of a bad RLE: %d %s", st, err.c_str());
            st = rle_draw::render_host(bset, images.data(), det.data(), min_score, alpha, stroke, rgb.data(), o_rgb.data(), &err);
            EXPECT(st == MRCNN_ERR_SHAPE && err.find(name) != std::string::npos && rgb == rgb0, "overlay of a bad RLE: %d %s", st, err.c_str());
        }
    }
    printf("%s: 3000 scenes, %d findings\n", findings ? "FAILED" : "clean", findings);
    return findings ? 1 : 0;
}
