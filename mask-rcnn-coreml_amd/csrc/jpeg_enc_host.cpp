// jpeg_enc_host.cpp — see jpeg_enc_host.h.  Plain C++17, no HIP.
#include "jpeg_enc_host.h"

#include <stdio.h>
#include <string.h>

#include <new>

#include "jpeg_math.h"

namespace mrcnn {
namespace jpeg {

namespace {

// ITU-T T.81 Annex K.1, natural order
const uint8_t kLumaQuant[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChromaQuant[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                  47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: the number of codes of each length 1..16, then the symbols in code order
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

struct HuffSource { const uint8_t* bits; const uint8_t* vals; int count; };
const HuffSource kDc[2] = {{kDcLumaBits, kDcVals, 12}, {kDcChromaBits, kDcVals, 12}};
const HuffSource kAc[2] = {{kAcLumaBits, kAcLumaVals, 162}, {kAcChromaBits, kAcChromaVals, 162}};

// the canonical codes of Annex C: counted up within a length, doubled from one length to the next
void derive(const HuffSource& s, uint32_t* entry)
{
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1] && k < s.count; ++i, ++k, ++code) entry[s.vals[k]] = (uint32_t)l << 16 | code;
        code <<= 1;
    }
}

void put16(std::vector<uint8_t>& o, int v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }

// The scan's bytes: bits MSB first, a zero byte after every FF
struct BitWriter {
    std::vector<uint8_t>& o;
    uint64_t acc = 0;           // the low `n` bits are pending
    int n = 0;
    void put(const Code& c)
    {
        for (int left = c.len; left > 0;) {                      // (<= 59 bits: in pieces that keep acc within 64)
            const int take = left < 32 ? left : 32;
            acc = (acc << take) | ((c.bits >> (left - take)) & ((1ull << take) - 1));
            n += take;
            left -= take;
            while (n >= 8) { emit((uint8_t)(acc >> (n - 8))); n -= 8; }
        }
    }
    void flush()                // the last byte is filled with 1-bits
    {
        if (n) emit((uint8_t)((acc << (8 - n)) | ((1u << (8 - n)) - 1)));
        n = 0;
    }
    void emit(uint8_t b)
    {
        o.push_back(b);
        if (b == 0xFF) o.push_back(0);
    }
};

}  // namespace

EncGeometry enc_geometry(int height, int width, int sampling)
{
    EncGeometry g;
    g.ncomp = sampling == ENC_GREY ? 1 : 3;
    g.hs = sampling == ENC_422 || sampling == ENC_420 ? 2 : 1;
    g.vs = sampling == ENC_420 ? 2 : 1;
    g.mcus_x = (width + 8 * g.hs - 1) / (8 * g.hs);
    g.mcus_y = (height + 8 * g.vs - 1) / (8 * g.vs);
    g.blocks_per_mcu = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    g.blocks = (int64_t)g.mcus_x * g.mcus_y * g.blocks_per_mcu;
    return g;
}

void enc_quant_tables(int quality, uint16_t quant[2][64])
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = ((t ? kChromaQuant[i] : kLumaQuant[i]) * scale + 50) / 100;
            quant[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

const EncHuffman& enc_huffman()
{
    static const EncHuffman table = [] {
        EncHuffman t;
        memset(&t, 0, sizeof t);
        for (int i = 0; i < 2; ++i) { derive(kDc[i], t.dc[i]); derive(kAc[i], t.ac[i]); }
        return t;
    }();
    return table;
}

std::vector<uint8_t> enc_header(int height, int width, int quality, int sampling)
{
    const EncGeometry g = enc_geometry(height, width, sampling);
    const int tables = g.ncomp == 1 ? 1 : 2;
    uint16_t quant[2][64];
    enc_quant_tables(quality, quant);
    std::vector<uint8_t> o;
    o.reserve(640);
    put16(o, 0xFFD8);
    put16(o, 0xFFE0); put16(o, 16);
    for (uint8_t b : {0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00}) o.push_back(b);
    put16(o, 0xFFDB); put16(o, 2 + 65 * tables);
    for (int t = 0; t < tables; ++t) {
        o.push_back((uint8_t)t);
        for (int k = 0; k < 64; ++k) o.push_back((uint8_t)quant[t][kZigzag[k]]);
    }
    put16(o, 0xFFC0); put16(o, 8 + 3 * g.ncomp);
    o.push_back(8); put16(o, height); put16(o, width); o.push_back((uint8_t)g.ncomp);
    for (int c = 0; c < g.ncomp; ++c) {
        o.push_back((uint8_t)(c + 1));
        o.push_back((uint8_t)(c == 0 ? (g.hs << 4 | g.vs) : 0x11));
        o.push_back((uint8_t)(c ? 1 : 0));
    }
    int dht = 2;
    for (int t = 0; t < tables; ++t) dht += 17 + kDc[t].count + 17 + kAc[t].count;
    put16(o, 0xFFC4); put16(o, dht);
    for (int t = 0; t < tables; ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const HuffSource& s = cls ? kAc[t] : kDc[t];
            o.push_back((uint8_t)(cls << 4 | t));
            o.insert(o.end(), s.bits, s.bits + 16);
            o.insert(o.end(), s.vals, s.vals + s.count);
        }
    put16(o, 0xFFDA); put16(o, 6 + 2 * g.ncomp);
    o.push_back((uint8_t)g.ncomp);
    for (int c = 0; c < g.ncomp; ++c) { o.push_back((uint8_t)(c + 1)); o.push_back((uint8_t)(c ? 0x11 : 0x00)); }
    o.push_back(0); o.push_back(63); o.push_back(0);
    return o;
}

int encode_host(const uint8_t* rgb, int height, int width, int quality, int sampling, uint8_t* out, int64_t capacity, int64_t* length,
                std::string* err)
{
    auto fail = [&](int code, const char* fmt, long long a, long long b) {
        if (err) { char buf[200]; snprintf(buf, sizeof buf, fmt, a, b); *err = buf; }
        return code;
    };
    if (!rgb || !length || capacity < 0 || (!out && capacity > 0)) return fail(MRCNN_ERR_INVALID, "jpeg_encode_host: null pointer or negative capacity", 0, 0);
    if (sampling < ENC_444 || sampling > ENC_GREY) return fail(MRCNN_ERR_INVALID, "jpeg_encode_host: unknown sampling %lld", sampling, 0);
    if (height < 1 || height > 32767 || width < 1 || width > 32767)
        return fail(MRCNN_ERR_SHAPE, "jpeg_encode_host: the image is %lldx%lld: height and width must lie in 1..32767", height, width);
    if (quality < 1 || quality > 100) return fail(MRCNN_ERR_SHAPE, "jpeg_encode_host: quality %lld outside 1..100", quality, 0);
    try {
        const EncGeometry g = enc_geometry(height, width, sampling);
        const EncHuffman& huff = enc_huffman();
        uint16_t quant[2][64];
        enc_quant_tables(quality, quant);
        std::vector<uint8_t> file = enc_header(height, width, quality, sampling);
        BitWriter bw{file};
        int pred[3] = {0, 0, 0};
        const int luma = g.ncomp == 1 ? 1 : g.hs * g.vs;
        for (int my = 0; my < g.mcus_y; ++my)
            for (int mx = 0; mx < g.mcus_x; ++mx)
                for (int k = 0; k < g.blocks_per_mcu; ++k) {
                    const int c = k < luma ? 0 : k - luma + 1;
                    const int bx = c ? mx : mx * g.hs + k % g.hs, by = c ? my : my * g.vs + k / g.hs;
                    int32_t ws[64];
                    for (int r = 0; r < 8; ++r) {
                        for (int i = 0; i < 8; ++i) ws[r * 8 + i] = enc_sample(rgb, height, width, sampling, c, bx * 8 + i, by * 8 + r) - 128;
                        fdct_1d(ws + r * 8, true);
                    }
                    for (int i = 0; i < 8; ++i) {
                        int32_t v[8];
                        for (int r = 0; r < 8; ++r) v[r] = ws[r * 8 + i];
                        fdct_1d(v, false);
                        for (int r = 0; r < 8; ++r) ws[r * 8 + i] = quantise(v[r], quant[c ? 1 : 0][r * 8 + i]);
                    }
                    const int t = c ? 1 : 0;
                    bw.put(code_dc(huff.dc[t], ws[0] - pred[c]));
                    pred[c] = ws[0];
                    int run = 0;
                    for (int z = 1; z < 64; ++z) {
                        const int32_t v = ws[kZigzag[z]];
                        if (v == 0) { ++run; continue; }
                        bw.put(code_ac(huff.ac[t], run, v));
                        run = 0;
                    }
                    if (run) bw.put(code_eob(huff.ac[t]));
                }
        bw.flush();
        file.push_back(0xFF); file.push_back(0xD9);
        *length = (int64_t)file.size();
        if (capacity == 0 && !out) return MRCNN_OK;
        if (capacity < *length)
            return fail(MRCNN_ERR_SHAPE, "jpeg_encode_host: the file needs %lld bytes, the buffer holds %lld", (long long)*length, (long long)capacity);
        memcpy(out, file.data(), file.size());
    } catch (const std::bad_alloc&) {
        return fail(MRCNN_ERR_INVALID, "jpeg_encode_host: out of memory encoding a %lldx%lld image", height, width);
    }
    return MRCNN_OK;
}

}  // namespace jpeg
}  // namespace mrcnn
