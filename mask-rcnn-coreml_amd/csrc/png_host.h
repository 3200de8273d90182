// png_host.h — the host half of the PNG encoder: the chunks before IDAT, CRC-32, and the sequential encoder that DEFINES the
// encoder's output (mrcnn_png_encode_host): the greedy parse of png_format.h's rule as it is stated, one token after another.  The
// kernels use the rule's closed form instead; the two meet in the files' bytes.  Plain C++17: no HIP header, builds with g++ alone
// (tools/png_check.cpp runs it under the sanitizers).  No codec is linked: the CRC is a table here, the Adler-32 a loop.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/maskrcnn_hip.h"

namespace mrcnn {
namespace png {

// zlib's convention: crc32(0, p, n) is the CRC of p[0 .. n), and crc32(that, q, k) continues it
uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n);

// everything of the file before IDAT's length: signature, IHDR, and for FORMAT_INSTANCE PLTE (rows + 1 entries) and tRNS (one byte)
std::vector<uint8_t> header(int height, int width, int format, int rows);

// an upper bound of the file's size: every raw byte a 9-bit literal
int64_t max_file_bytes(int height, int width, size_t header_bytes);

// The argument checks both entries share; `who` starts the message ("png_encode_host", "png_encode_batch: image 3 of the batch").
// check_format: unknown format -> MRCNN_ERR_INVALID, (INSTANCE) rows outside 1..255 -> MRCNN_ERR_SHAPE.
// check_image:  null pixels -> MRCNN_ERR_INVALID, a side outside 1..32767 -> MRCNN_ERR_SHAPE.
int check_format(int format, int rows, const char* who, std::string* err);
int check_image(const void* pixels, int height, int width, const char* who, std::string* err);

// The whole encoder on the host.  *length is always the size needed; out may be NULL when capacity is 0 (the size query);
// capacity < *length -> MRCNN_ERR_SHAPE and out is not written.
int encode_host(const void* pixels, int height, int width, int format, int rows, uint8_t* out, int64_t capacity, int64_t* length,
                std::string* err);

}  // namespace png
}  // namespace mrcnn
