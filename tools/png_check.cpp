// png_check.cpp — the host PNG encoder (csrc/png_host.cpp) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc
//       tools/png_check.cpp mask-rcnn-coreml_amd/csrc/png_host.cpp -o png_check            (one command line)
//   ./png_check
//
// Host code only: no GPU, no HIP, no Python, no zlib.  It sweeps every size 1x1 .. 40x40 and the sizes around the 4096-byte deflate
// block (N = 4096, 4097, 6144, 8192, and a row of runs of every length-code boundary), both formats, over seeded images: noise (9-bit
// literals), blobs (long runs) and zeros.  Each image is encoded three times — the size query, a buffer one byte short, a buffer of
// exactly the size reported (so a write past it is a report).  The file is then taken apart by the small inflater below (fixed
// Huffman blocks only, written from RFC 1951, sharing nothing with png_format.h) and compared with the raw stream R rebuilt here;
// the chunk CRCs are checked bit by bit and the Adler-32 byte by byte.  Last, the rule's closed form (png_format.h segment_token,
// what the kernels run) is replayed position by position and must give the definition's deflate stream.  Exit status: 0 = clean;
// 1 = a finding; a sanitizer report ends the program with the sanitizer's own non-zero status.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "png_format.h"
#include "png_host.h"

using namespace mrcnn;

namespace {

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

uint32_t crc_bitwise(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

// RFC 1951: fixed-Huffman blocks only.  false = a malformed stream, another block type, or a read past the end.
struct Inflater {
    const uint8_t* p;
    size_t n, bit = 0;
    bool ok = true;
    int get()
    {
        if (bit >= n * 8) { ok = false; return 0; }
        const int b = p[bit >> 3] >> (bit & 7) & 1;
        ++bit;
        return b;
    }
    int value(int len) { int v = 0; for (int k = 0; k < len; ++k) v |= get() << k; return v; }          // least significant bit first
    int code(int len) { int v = 0; for (int k = 0; k < len; ++k) v = v << 1 | get(); return v; }        // Huffman: most significant first
    int symbol()
    {
        int c = code(7);
        if (c <= 0x17) return 256 + c;
        c = c << 1 | get();
        if (c >= 0x30 && c <= 0xBF) return c - 0x30;
        if (c >= 0xC0 && c <= 0xC7) return 280 + c - 0xC0;
        c = c << 1 | get();
        return c >= 0x190 ? 144 + c - 0x190 : -1;
    }
    bool run(std::vector<uint8_t>& out, int* blocks, size_t* end_byte)
    {
        static const int len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const int len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static const int dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        static const int dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        *blocks = 0;
        for (int final = 0; !final && ok;) {
            final = get();
            if (value(2) != 1) return false;
            ++*blocks;
            for (;;) {
                const int s = symbol();
                if (!ok || s < 0 || s > 285) return false;
                if (s == 256) break;
                if (s < 256) { out.push_back((uint8_t)s); continue; }
                const int length = len_base[s - 257] + value(len_extra[s - 257]), d = code(5);
                if (d > 29) return false;
                const size_t distance = (size_t)dist_base[d] + (size_t)value(dist_extra[d]);
                if (distance > out.size()) return false;
                for (int k = 0; k < length; ++k) out.push_back(out[out.size() - distance]);
            }
        }
        *end_byte = (bit + 7) / 8;
        return ok;
    }
};

// the deflate stream of `raw` from the closed form: what a lane of kernels_png.hip does for its position, one position after another
std::vector<uint8_t> closed_form_stream(const std::vector<uint8_t>& raw)
{
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    int pending = 0;
    auto put = [&](uint32_t bits, int len) {
        acc |= (uint64_t)bits << pending;
        pending += len;
        while (pending >= 8) { out.push_back((uint8_t)acc); acc >>= 8; pending -= 8; }
    };
    const int64_t n = (int64_t)raw.size();
    for (int64_t b0 = 0; b0 < n; b0 += png::PNG_BLOCK_BYTES) {
        const int64_t b1 = b0 + png::PNG_BLOCK_BYTES < n ? b0 + png::PNG_BLOCK_BYTES : n;
        put(png::block_header(b1 == n), png::BLOCK_HEADER_BITS);
        auto equal = [&](int64_t p) { return p > 0 && raw[(size_t)p] == raw[(size_t)p - 1]; };
        for (int64_t p = b0; p < b1; ++p) {
            int kind = 1;
            if (equal(p)) {
                int64_t start = p, end = p + 1;
                while (start > b0 && equal(start - 1)) --start;
                while (end < b1 && equal(end)) ++end;
                kind = png::segment_token((int)(p - start), (int)(end - start));
            }
            if (kind == 0) continue;
            const png::Token t = kind == 1 ? png::literal_token(raw[(size_t)p]) : png::match_token(kind);
            put(t.bits, t.len);
        }
        put(0, png::END_OF_BLOCK_BITS);
    }
    if (pending) out.push_back((uint8_t)acc);
    return out;
}

struct Shape { int h, w; };

}  // namespace

int main()
{
    int bad = 0;
    long runs = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    std::vector<Shape> shapes;
    for (int h = 1; h <= 40; ++h)
        for (int w = 1; w <= 40; ++w) shapes.push_back({h, w});
    for (Shape s : {Shape{1, 4095}, Shape{1, 4096}, Shape{2, 4095}, Shape{3, 2047}, Shape{1, 2857}, Shape{70, 61}}) shapes.push_back(s);
    static const int run_lengths[12] = {1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519};

    for (const Shape& s : shapes)
        for (int format = 0; format < 2; ++format)
            for (int content = 0; content < 3; ++content) {
                const int h = s.h, w = s.w, rows = format ? (content == 0 ? 255 : 1 + (h + w) % 255) : 0;
                const size_t count = (size_t)h * w;
                // exact-size copies of the pixels: a read past h*w samples is a read past the allocation
                std::vector<uint8_t> grey(format ? 0 : count);
                std::vector<int16_t> ids(format ? count : 0);
                uint32_t value = next() & 255u;
                size_t left = 0, k = 0;
                for (size_t i = 0; i < count; ++i) {
                    uint32_t v;
                    if (content == 0) v = next() & 511u;                                       // noise (an int16 map: ids above rows too)
                    else if (content == 2) v = 0;
                    else {                                                                     // runs: the length-code boundaries in turn, a new value each
                        if (left == 0) { left = (size_t)run_lengths[k++ % 12]; value = (value + 1 + next() % 200u) & 255u; }
                        --left;
                        v = value;
                    }
                    if (format) ids[i] = (int16_t)((int)v - 2); else grey[i] = (uint8_t)v;
                }
                const void* pixels = format ? (const void*)ids.data() : (const void*)grey.data();
                ++runs;
                std::string err;
                int64_t need = -1, n = -1;
                if (png::encode_host(pixels, h, w, format, rows, nullptr, 0, &need, &err) != MRCNN_OK || need < 67) {   // (a 1x1 grey file is 67 bytes)
                    printf("%dx%d f%d c%d: size query failed (%s)\n", h, w, format, content, err.c_str());
                    ++bad;
                    continue;
                }
                std::vector<uint8_t> small((size_t)need - 1, 0xAB);
                if (png::encode_host(pixels, h, w, format, rows, small.data(), need - 1, &n, &err) != MRCNN_ERR_SHAPE || n != need || small[0] != 0xAB ||
                    small.back() != 0xAB) {
                    printf("%dx%d f%d c%d: a buffer one byte short was not refused untouched\n", h, w, format, content);
                    ++bad;
                }
                std::vector<uint8_t> file((size_t)need);
                if (png::encode_host(pixels, h, w, format, rows, file.data(), need, &n, &err) != MRCNN_OK || n != need ||
                    need > png::max_file_bytes(h, w, png::header(h, w, format, rows).size())) {
                    printf("%dx%d f%d c%d: encode failed or the file is over the bound (%s)\n", h, w, format, content, err.c_str());
                    ++bad;
                    continue;
                }
                // R, rebuilt here
                std::vector<uint8_t> raw;
                for (int y = 0; y < h; ++y) {
                    raw.push_back(0);
                    for (int x = 0; x < w; ++x) {
                        const size_t i = (size_t)y * w + x;
                        raw.push_back(format ? (uint8_t)(ids[i] >= -1 && ids[i] < rows ? ids[i] + 1 : 0) : grey[i]);
                    }
                }
                // the chunks: their order, their CRCs, and IDAT
                std::string order;
                const uint8_t* idat = nullptr;
                size_t idat_len = 0, at = 8;
                bool framed = need >= 8 && memcmp(file.data(), "\x89PNG\r\n\x1a\n", 8) == 0;
                while (framed && at + 12 <= file.size()) {
                    const size_t len = be32(&file[at]);
                    if (at + 12 + len > file.size()) { framed = false; break; }
                    if (crc_bitwise(&file[at + 4], len + 4) != be32(&file[at + 8 + len])) framed = false;
                    order += std::string((const char*)&file[at + 4], 4) + " ";
                    if (memcmp(&file[at + 4], "IDAT", 4) == 0) { idat = &file[at + 8]; idat_len = len; }
                    at += 12 + len;
                }
                if (!framed || at != file.size() || order != (format ? "IHDR PLTE tRNS IDAT IEND " : "IHDR IDAT IEND ") || !idat || idat_len < 6 || idat[0] != 0x78 ||
                    idat[1] != 0x01) {
                    printf("%dx%d f%d c%d: the chunks are not as documented (%s)\n", h, w, format, content, order.c_str());
                    ++bad;
                    continue;
                }
                std::vector<uint8_t> back;
                int blocks = 0;
                size_t end_byte = 0;
                Inflater z{idat + 2, idat_len - 6};
                uint32_t a = 1, b = 0;
                for (uint8_t v : raw) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
                if (!z.run(back, &blocks, &end_byte) || back != raw || end_byte != idat_len - 6 || blocks != (int)((raw.size() + 4095) / 4096) ||
                    be32(idat + idat_len - 4) != (b << 16 | a)) {
                    printf("%dx%d f%d c%d: the stream does not inflate to R in %d blocks, or the Adler-32 is off\n", h, w, format, content, (int)((raw.size() + 4095) / 4096));
                    ++bad;
                    continue;
                }
                const std::vector<uint8_t> closed = closed_form_stream(raw);
                if (closed.size() != idat_len - 6 || memcmp(closed.data(), idat + 2, closed.size()) != 0) {
                    printf("%dx%d f%d c%d: the closed form gives another stream than the greedy parse\n", h, w, format, content);
                    ++bad;
                }
            }
    printf("%ld encodes, %d findings\n", runs, bad);
    return bad ? 1 : 0;
}
