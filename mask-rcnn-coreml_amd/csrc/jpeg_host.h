// jpeg_host.h — the serial half of the JPEG decoder: marker parsing, Huffman table construction and the entropy decoder, plus the
// scalar pipeline that DEFINES the decoder's output (mrcnn_jpeg_decode_host).  Plain C++17: no HIP header, builds with g++ alone
// (tools/jpeg_host_check.cpp runs it under the sanitizers).  Every function returns an MRCNN_* status and, on failure, says why in *err.
//
// Scope: baseline sequential DCT (SOF0), 8-bit, Huffman, ONE interleaved scan; 1 component (grey) or 3 (YCbCr) sampled 4:4:4,
// 4:2:2 (h2v1) or 4:2:0 (h2v2); 8- and 16-bit quantisation tables, any DHT, restart intervals.  Anything else -> MRCNN_ERR_UNSUPPORTED
// naming what was found; a damaged or truncated stream -> MRCNN_ERR_IO.  Every read is checked against `length`.
#pragma once
#include <stdint.h>
#include <string>

#include "../../include/maskrcnn_hip.h"
#include "jpeg_huff.h"

namespace mrcnn {
namespace jpeg {

struct Component {
    int id, h_samp, v_samp, tq, td, ta;
    int width, height;          // the component's own (downsampled) size in samples: ceil(image * samp / max_samp)
    int blocks_w, blocks_h;     // its block grid, padded to whole MCUs
    int64_t block0;             // first block of this component in the image's coefficient array
};

struct HuffSpec {
    bool defined;
    uint8_t bits[17];           // bits[l] = number of codes of length l (1..16)
    uint8_t vals[256];
    int count;
};

struct Header {
    int height, width, components;
    int h_samp, v_samp;         // of the first component (1 for a one-component file)
    int mode;                   // jpeg_math.h MODE_*
    int mcus_x, mcus_y, restart_interval;
    Component comp[3];
    uint16_t quant[4][64];      // natural (row-major) order
    bool quant_defined[4];
    HuffSpec dc[4], ac[4];
    int64_t scan_offset;        // first byte of entropy-coded data
    int64_t total_blocks;       // over all components: the coefficient array holds total_blocks * 64 int16
};

// Parses every segment up to and including SOS and validates the file against the scope above.  Reads nothing behind the SOS header.
int parse(const uint8_t* data, int64_t length, Header* out, std::string* err);

// The decoding table of a DHT table the parser accepted: for decode_coefficients and for the entropy stage's plan (jpeg_entropy_host.h).
void build_huff_table(const HuffSpec& s, HuffTable& t);

// Entropy-decodes the scan into coef[total_blocks * 64] (natural order within a block; component c's blocks start at comp[c].block0,
// row-major over its padded grid).  The array is cleared here.  The scan must be followed by EOI.
int decode_coefficients(const uint8_t* data, int64_t length, const Header& h, int16_t* coef, std::string* err);

// The whole pipeline on the host: parse, entropy-decode, dequantise + IDCT, upsample, colour -> rgb[height * width * 3].
// capacity < height * width * 3 -> MRCNN_ERR_SHAPE.
int decode_host(const uint8_t* data, int64_t length, uint8_t* rgb, int64_t capacity, std::string* err);

}  // namespace jpeg
}  // namespace mrcnn
