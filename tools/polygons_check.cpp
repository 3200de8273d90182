// polygons_check.cpp — the host definition of mrcnn_rle_to_polygons (csrc/polygons_host.cpp) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc tools/polygons_check.cpp
//       mask-rcnn-coreml_amd/csrc/polygons_host.cpp mask-rcnn-coreml_amd/csrc/rle_draw_host.cpp mask-rcnn-coreml_amd/csrc/rle_set_host.cpp
//       -o polygons_check                                                                            (one command line)
//   ./polygons_check
//
// Host code only: no GPU, no HIP, no Python.  3 000 seeded sets — one to three images of 1x1 .. 17x17, one to four slots, random runs
// with zero-length runs thrown in anywhere and runs of ones across column ends — are traced; the signed areas must sum to the set pixels
// and the offsets must end at the vertices.  Now and then one count is moved by one: MRCNN_ERR_SHAPE, and the output stays as it was.
#include <cstdio>
#include <random>
#include <vector>
#include "polygons_host.h"
using namespace mrcnn;
int main()
{
    std::mt19937 rng(7);
    long rings = 0, verts = 0;
    for (int it = 0; it < 3000; ++it) {
        const int B = 1 + rng() % 3, slots = 1 + rng() % 4;
        std::vector<int32_t> hs(B), ws(B);
        std::vector<uint32_t> counts; std::vector<int64_t> offs{0};
        long want_area = 0;
        for (int b = 0; b < B; ++b) {
            hs[b] = 1 + rng() % 17; ws[b] = 1 + rng() % 17;
            for (int i = 0; i < slots; ++i) {
                uint32_t left = (uint32_t)hs[b] * ws[b]; int j = 0;
                while (left) { uint32_t c = rng() % 5 == 0 ? 0 : 1 + rng() % (1 + left / (1 + rng() % 8)); if (c > left) c = left; counts.push_back(c); if (j & 1) want_area += c; left -= c; ++j; }
                if (rng() % 3 == 0) counts.push_back(0);
                offs.push_back((int64_t)counts.size());
            }
        }
        rle_draw::Set s{counts.data(), offs.data(), B, slots, hs.data(), ws.data()};
        polygons::Rings r; std::string err;
        if (polygons::trace_host(s, "check", &r, &err) != 0) { printf("FAIL %s\n", err.c_str()); return 1; }
        long a = 0; for (auto v : r.ring_areas) a += v;
        if (a != want_area || r.ring_offsets.back() != (int64_t)r.xy.size() / 2) { printf("area mismatch %ld %ld\n", a, want_area); return 1; }
        rings += (long)r.ring_areas.size(); verts += (long)r.xy.size() / 2;
        if (it % 500 == 0 && !counts.empty()) {            // a bad RLE: refused, out untouched
            counts[0] += 1; polygons::Rings q; q.xy.push_back(42);
            if (polygons::trace_host(s, "check", &q, &err) != MRCNN_ERR_SHAPE || q.xy.size() != 1) { printf("bad RLE not refused\n"); return 1; }
        }
    }
    printf("ok: %ld rings, %ld vertices\n", rings, verts);
    return 0;
}
