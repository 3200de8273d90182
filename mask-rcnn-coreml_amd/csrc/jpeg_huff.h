// jpeg_huff.h — what every JPEG translation unit here agrees on, written once: the zigzag order, the Huffman decoding table and its
// lookup.  The sequential decoder (jpeg_host.cpp), the entropy stage's step function (jpeg_entropy.h: the kernels and the host model)
// and the encoder (jpeg_enc_host.cpp, api_jpeg_enc.hip) all read these.  Plain C++: no HIP header, g++ builds it alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_HUFF_HD __host__ __device__ inline
#else
#define MRCNN_HUFF_HD inline
#endif

namespace mrcnn {
namespace jpeg {

// zigzag position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A DHT table ready for decoding (jpeg_host.h's build_huff_table), self-contained: what a workgroup copies into LDS, 356 words
struct HuffTable {
    uint16_t look[512];         // 9 leading bits -> (length << 8) | symbol, 0 = longer than 9 bits (or no such code)
    int32_t maxcode[18];        // largest code of each length, -1 = none
    int32_t valoff[17];         // index of a length's first symbol minus its first code
    int32_t count;
    uint8_t vals[256];
};
static_assert(sizeof(HuffTable) == 1424, "HuffTable is copied as 356 words");

// The code that opens the next 32 bits of the stream `w` (MSB first): (length << 8) | symbol, 0 = no such code.
MRCNN_HUFF_HD int huff_lookup(const HuffTable& t, uint32_t w)
{
    const int e = t.look[w >> 23];
    if (e) return e;
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(w >> (32 - l));
        if (code <= t.maxcode[l]) {
            const int idx = code + t.valoff[l];
            return idx < 0 || idx >= t.count ? 0 : (l << 8) | t.vals[idx];
        }
    }
    return 0;
}

}  // namespace jpeg
}  // namespace mrcnn
