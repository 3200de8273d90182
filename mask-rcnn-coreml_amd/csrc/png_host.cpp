// png_host.cpp — see png_host.h.  Plain C++17, no HIP.
#include "png_host.h"

#include <stdio.h>
#include <string.h>

#include <new>

#include "png_format.h"

namespace mrcnn {
namespace png {

namespace {

struct CrcTable {
    uint32_t t[256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
};

void put32(std::vector<uint8_t>& o, uint32_t v)
{
    o.push_back((uint8_t)(v >> 24)); o.push_back((uint8_t)(v >> 16)); o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v);
}

// length, type, data, CRC of type + data
void put_chunk(std::vector<uint8_t>& o, const char* type, const std::vector<uint8_t>& data)
{
    put32(o, (uint32_t)data.size());
    const size_t at = o.size();
    o.insert(o.end(), type, type + 4);
    o.insert(o.end(), data.begin(), data.end());
    put32(o, crc32(0, o.data() + at, o.size() - at));
}

// The deflate stream's bytes: bits least significant first
struct BitWriter {
    std::vector<uint8_t>& o;
    uint64_t acc = 0;           // the low `n` bits are pending
    int n = 0;
    void put(uint32_t bits, int len)
    {
        acc |= (uint64_t)bits << n;
        n += len;
        while (n >= 8) { o.push_back((uint8_t)acc); acc >>= 8; n -= 8; }
    }
    void flush() { if (n) { o.push_back((uint8_t)acc); acc = 0; n = 0; } }       // the last byte zero-padded
};

int set_err(std::string* err, int code, const char* fmt, const char* who, long long a, long long b)
{
    if (err) { char buf[240]; snprintf(buf, sizeof buf, fmt, who, a, b); *err = buf; }
    return code;
}

}  // namespace

uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n)
{
    static const CrcTable table;
    uint32_t c = ~crc;
    for (size_t i = 0; i < n; ++i) c = table.t[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

std::vector<uint8_t> header(int height, int width, int format, int rows)
{
    static const uint8_t signature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::vector<uint8_t> o(signature, signature + 8), d;
    put32(d, (uint32_t)width); put32(d, (uint32_t)height);
    d.push_back(8);                                              // bit depth
    d.push_back(format == FORMAT_INSTANCE ? 3 : 0);              // colour type: palette / greyscale
    d.push_back(0); d.push_back(0); d.push_back(0);              // deflate, adaptive filtering (every row type 0), no interlace
    put_chunk(o, "IHDR", d);
    if (format == FORMAT_INSTANCE) {
        d.assign(3, 0);
        for (int k = 1; k <= rows; ++k) {
            const uint32_t c = palette_rgb(k - 1);
            d.push_back((uint8_t)(c >> 16)); d.push_back((uint8_t)(c >> 8)); d.push_back((uint8_t)c);
        }
        put_chunk(o, "PLTE", d);
        d.assign(1, 0);                                          // index 0 transparent, every other entry opaque
        put_chunk(o, "tRNS", d);
    }
    return o;
}

int64_t max_file_bytes(int height, int width, size_t header_bytes)
{
    const int64_t n = (int64_t)height * (width + 1), blocks = (n + PNG_BLOCK_BYTES - 1) / PNG_BLOCK_BYTES;
    return (int64_t)header_bytes + IDAT_LEAD + (n * 9 + blocks * (BLOCK_HEADER_BITS + END_OF_BLOCK_BITS) + 7) / 8 + IDAT_TAIL + IEND_BYTES;
}

int check_format(int format, int rows, const char* who, std::string* err)
{
    if (format != FORMAT_GREY8 && format != FORMAT_INSTANCE) return set_err(err, MRCNN_ERR_INVALID, "%s: unknown format %lld", who, format, 0);
    if (format == FORMAT_INSTANCE && (rows < 1 || rows > 255))
        return set_err(err, MRCNN_ERR_SHAPE, "%s: rows %lld outside 1..255 (an INSTANCE file has 8-bit indices)", who, rows, 0);
    return MRCNN_OK;
}

int check_image(const void* pixels, int height, int width, const char* who, std::string* err)
{
    if (!pixels) return set_err(err, MRCNN_ERR_INVALID, "%s: null pixels", who, 0, 0);
    if (height < 1 || height > 32767 || width < 1 || width > 32767)
        return set_err(err, MRCNN_ERR_SHAPE, "%s is %lldx%lld: height and width must lie in 1..32767", who, height, width);
    return MRCNN_OK;
}

int encode_host(const void* pixels, int height, int width, int format, int rows, uint8_t* out, int64_t capacity, int64_t* length,
                std::string* err)
{
    if (!length || capacity < 0 || (!out && capacity > 0)) return set_err(err, MRCNN_ERR_INVALID, "%s: null pointer or negative capacity", "png_encode_host", 0, 0);
    if (const int st = check_format(format, rows, "png_encode_host", err)) return st;
    if (const int st = check_image(pixels, height, width, "png_encode_host: the image", err)) return st;
    try {
        const int64_t n = (int64_t)height * (width + 1);
        std::vector<uint8_t> raw((size_t)n);
        for (int y = 0; y < height; ++y) {
            uint8_t* line = raw.data() + (size_t)y * (width + 1);
            line[0] = 0;
            for (int x = 0; x < width; ++x) line[1 + x] = (uint8_t)sample_byte(pixels, (long long)y * width + x, format, rows);
        }
        std::vector<uint8_t> file = header(height, width, format, rows);
        const size_t idat = file.size();
        put32(file, 0);                                          // IDAT's length, known at the end
        file.insert(file.end(), {'I', 'D', 'A', 'T', 0x78, 0x01});
        BitWriter bw{file};
        for (int64_t b0 = 0; b0 < n; b0 += PNG_BLOCK_BYTES) {
            const int64_t b1 = b0 + PNG_BLOCK_BYTES < n ? b0 + PNG_BLOCK_BYTES : n;
            bw.put(block_header(b1 == n), BLOCK_HEADER_BITS);
            for (int64_t p = b0; p < b1;) {
                const int64_t most = b1 - p < (int64_t)MAX_MATCH ? b1 - p : (int64_t)MAX_MATCH;
                int64_t run = 0;
                while (p > 0 && run < most && raw[(size_t)(p + run)] == raw[(size_t)(p + run - 1)]) ++run;
                if (run >= MIN_MATCH) {
                    const Token t = match_token((int)run);
                    bw.put(t.bits, t.len);
                    p += run;
                } else {
                    const Token t = literal_token(raw[(size_t)p]);
                    bw.put(t.bits, t.len);
                    p += 1;
                }
            }
            bw.put(0, END_OF_BLOCK_BITS);
        }
        bw.flush();
        uint32_t a = 1, b = 0;
        for (int64_t p = 0; p < n;) {                            // (5552 bytes keep b inside 32 bits)
            const int64_t stop = p + 5552 < n ? p + 5552 : n;
            for (; p < stop; ++p) { a += raw[(size_t)p]; b += a; }
            a %= ADLER_MOD; b %= ADLER_MOD;
        }
        put32(file, b << 16 | a);
        const uint32_t data_bytes = (uint32_t)(file.size() - idat - 8);
        for (int k = 0; k < 4; ++k) file[idat + k] = (uint8_t)(data_bytes >> (24 - 8 * k));
        put32(file, crc32(0, file.data() + idat + 4, file.size() - idat - 4));
        put_chunk(file, "IEND", std::vector<uint8_t>());
        *length = (int64_t)file.size();
        if (capacity == 0 && !out) return MRCNN_OK;
        if (capacity < *length)
            return set_err(err, MRCNN_ERR_SHAPE, "%s: the file needs %lld bytes, the buffer holds %lld", "png_encode_host", (long long)*length, (long long)capacity);
        memcpy(out, file.data(), file.size());
    } catch (const std::bad_alloc&) {
        return set_err(err, MRCNN_ERR_INVALID, "%s: out of memory encoding a %lldx%lld image", "png_encode_host", height, width);
    }
    return MRCNN_OK;
}

}  // namespace png
}  // namespace mrcnn
