// jpeg_enc_host.h — the host half of the JPEG encoder: the tables (Annex K quantisation scaled by libjpeg's quality rule, the four
// standard Huffman tables as code words), the file header, and the scalar pipeline that DEFINES the encoder's output
// (mrcnn_jpeg_encode_host).  Plain C++17: no HIP header, builds with g++ alone (tools/jpeg_enc_check.cpp runs it under the sanitizers).
//
// The file: baseline sequential (SOF0), 8-bit, one interleaved scan; SOI, JFIF APP0 (1.1, density 1:1, no units), DQT, SOF0, DHT, SOS,
// the scan, EOI.  Not written: restart markers, optimised Huffman tables, progressive scans.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/maskrcnn_hip.h"
#include "jpeg_huff.h"

namespace mrcnn {
namespace jpeg {

struct EncGeometry {
    int ncomp;                  // 1 (grey) or 3
    int hs, vs;                 // luma sampling factors; the chroma components are 1x1
    int mcus_x, mcus_y;
    int blocks_per_mcu;         // hs * vs luma blocks, then one Cb, one Cr
    int64_t blocks;             // mcus_x * mcus_y * blocks_per_mcu, in scan order
};
EncGeometry enc_geometry(int height, int width, int sampling);

// tables 0 (luma) and 1 (chroma) for `quality` 1..100, natural order, entries 1..255
void enc_quant_tables(int quality, uint16_t quant[2][64]);

// entry[symbol] = length << 16 | code (jpeg_math.h code_dc / code_ac); [0] luma, [1] chroma
struct EncHuffman {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
const EncHuffman& enc_huffman();

// everything of the file before the scan's first byte
std::vector<uint8_t> enc_header(int height, int width, int quality, int sampling);

// The whole encoder on the host.  *length is always the size needed; out may be NULL when capacity is 0 (the size query);
// capacity < *length -> MRCNN_ERR_SHAPE and out is not written.
int encode_host(const uint8_t* rgb, int height, int width, int quality, int sampling, uint8_t* out, int64_t capacity, int64_t* length,
                std::string* err);

}  // namespace jpeg
}  // namespace mrcnn
