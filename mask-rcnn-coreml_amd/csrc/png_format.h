// png_format.h — the PNG encoder's format, written once for the host definition (png_host.cpp, plain C++) and for the kernels
// (kernels_png.hip): the raw stream's bytes, the token the rule puts at a position, and its fixed-Huffman bits.  No HIP header is
// included here.
//
// The file (include/maskrcnn_hip.h has the caller's view): signature, IHDR, [PLTE, tRNS], ONE IDAT, IEND.  The raw stream R is, per
// scanline, one filter byte 0 and the w sample bytes: N = h (w + 1).  IDAT = 78 01, a deflate stream, Adler-32 of R.  The deflate
// stream cuts R into blocks of PNG_BLOCK_BYTES raw bytes, each ONE fixed-Huffman block (BFINAL on the last, BTYPE 01, tokens, end of
// block), bit-contiguous, the last byte zero-padded.  The tokens are zlib's Z_RLE matcher, distance 1 only — for a block [b0, b1) and
// p from b0: n = the number of k >= 0 with R[p+k] == R[p+k-1], counted up to min(258, b1 - p), 0 at p = 0; n >= 3 emits (length n,
// distance 1) and p += n, else the literal R[p] and p += 1.  A match may reach back over the block's start and never runs over its end,
// so blocks are independent.  The rule has a closed form per position (segment_token below), so the device parses nothing sequentially.
//
// Left out on purpose: RGB8, 16-bit samples, interlacing, dynamic Huffman tables, decoding — and row filters other than 0, which gain
// nothing on label data under this matcher (a 240x320 map of 12 blobs: filter 0 -> 3 666 B, Up -> 3 818 B, Sub -> 5 728 B, 77 040 B
// raw).  Photographs come out LARGER than raw with fixed codes; pictures have the JPEG encoder.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_PNG_HD __host__ __device__ inline
#else
#define MRCNN_PNG_HD inline
#endif

namespace mrcnn {
namespace png {

enum { FORMAT_GREY8 = 0, FORMAT_INSTANCE = 1 };         // MRCNN_PNG_GREY8 / MRCNN_PNG_INSTANCE
enum { PNG_BLOCK_BYTES = 4096, MAX_MATCH = 258, MIN_MATCH = 3 };
enum { ADLER_MOD = 65521 };
// what follows the host-built chunks in a file: IDAT's length and type, 78 01 | deflate | Adler-32, IDAT's CRC, IEND
enum { IDAT_LEAD = 10, IDAT_TAIL = 8, IEND_BYTES = 12 };

// entry k >= 1 of an INSTANCE file's PLTE is palette_rgb(k - 1) — red, blue, green, yellow: DetectionRenderer.swift:53, the colour
// mrcnn_render_detections_source gives row k - 1; entry 0 ("no detection") is black and, by tRNS, transparent
MRCNN_PNG_HD uint32_t palette_rgb(int row)              // 0xRRGGBB
{
    const int k = row & 3;
    return k == 0 ? 0xFF0000u : k == 1 ? 0x0000FFu : k == 2 ? 0x00FF00u : 0xFFFF00u;
}

// the sample byte of pixel i: GREY8 as it is; INSTANCE v + 1 for v in -1 .. rows - 1, any other value 0
MRCNN_PNG_HD uint32_t sample_byte(const void* pixels, long long i, int format, int rows)
{
    if (format == FORMAT_GREY8) return static_cast<const uint8_t*>(pixels)[i];
    const int v = static_cast<const int16_t*>(pixels)[i];
    return v >= -1 && v < rows ? (uint32_t)(v + 1) : 0u;
}

// R[p], 0 <= p < h (w + 1) — below 2^30 for sides up to 32767, so the division is a 32-bit one
MRCNN_PNG_HD uint32_t raw_byte(const void* pixels, int w, long long p, int format, int rows)
{
    const uint32_t row = (uint32_t)p / (uint32_t)(w + 1), col = (uint32_t)p - row * (uint32_t)(w + 1);
    return col == 0 ? 0u : sample_byte(pixels, (long long)row * w + col - 1, format, rows);
}

// `len` bits, to be written least significant bit first
struct Token { uint32_t bits; int len; };

MRCNN_PNG_HD uint32_t reverse_bits(uint32_t x, int len)  // the low `len` (1..16) bits of x in the opposite order
{
    x = (x & 0x5555u) << 1 | (x >> 1 & 0x5555u);
    x = (x & 0x3333u) << 2 | (x >> 2 & 0x3333u);
    x = (x & 0x0F0Fu) << 4 | (x >> 4 & 0x0F0Fu);
    x = (x & 0x00FFu) << 8 | (x >> 8 & 0x00FFu);
    return x >> (16 - len);
}

// RFC 1951 3.2.6, the fixed code of literal / length symbol 0..287; Huffman codes go out most significant bit first, so reversed here
MRCNN_PNG_HD Token fixed_code(int symbol)
{
    Token t;
    if (symbol < 144) { t.len = 8; t.bits = reverse_bits(0x30u + symbol, 8); }
    else if (symbol < 256) { t.len = 9; t.bits = reverse_bits(0x190u + (symbol - 144), 9); }
    else if (symbol < 280) { t.len = 7; t.bits = reverse_bits((uint32_t)(symbol - 256), 7); }
    else { t.len = 8; t.bits = reverse_bits(0xC0u + (symbol - 280), 8); }
    return t;
}

MRCNN_PNG_HD Token literal_token(uint32_t byte) { return fixed_code((int)byte); }

// (length 3..258, distance 1): the length symbol 257..285 (3.2.5: eight lengths a symbol-group of 4, each group one more extra bit;
// 258 alone is 285), its extra bits as they are, then the 5-bit distance code 0 — at most 8 + 5 + 5 = 18 bits
MRCNN_PNG_HD Token match_token(int length)
{
    const int l = length - MIN_MATCH;
    int symbol = 285, extra_bits = 0;
    if (l < 8) symbol = 257 + l;
    else if (length < MAX_MATCH) {
        int top = 3;                                     // floor(log2(l)), l in 8..254
        while ((l >> (top + 1)) != 0) ++top;
        extra_bits = top - 2;
        symbol = 257 + 4 * extra_bits + 4 + ((l >> extra_bits) & 3);
    }
    Token t = fixed_code(symbol);
    t.bits |= (uint32_t)(l & ((1 << extra_bits) - 1)) << t.len;
    t.len += extra_bits + 5;
    return t;
}

enum { BLOCK_HEADER_BITS = 3, END_OF_BLOCK_BITS = 7 };   // BFINAL + BTYPE 01 (value 2 | final, LSB first); symbol 256 = 0000000
MRCNN_PNG_HD uint32_t block_header(bool final) { return 2u | (final ? 1u : 0u); }

// The closed form of the rule.  Position j (from 0) of a maximal segment of m positions with R[p] == R[p-1], clipped to the block:
// m / 258 full matches, then one match of m % 258 if that is >= 3, else that many literals.  Returns the length of the match that
// STARTS at j, 1 for a literal, 0 when j lies inside a match.  (A position outside such a segment is a literal.)
MRCNN_PNG_HD int segment_token(int j, int m)
{
    const int full = m / MAX_MATCH * MAX_MATCH, rest = m - full;
    if (j < full) return j % MAX_MATCH == 0 ? MAX_MATCH : 0;
    if (rest >= MIN_MATCH) return j == full ? rest : 0;
    return 1;
}

// Adler-32 from per-block sums: a block [b0, b1) of an N-byte stream with S1 = sum R[p] and S2 = sum (b1 - p) R[p] adds S1 to `a` and
// S2 + (N - b1) S1 to `b`, on top of a = 1, b = N (every byte of the stream sees the initial 1).  Both reduced, so sums of them over
// any number of blocks stay far inside 64 bits.
MRCNN_PNG_HD uint32_t adler_block_a(unsigned long long s1) { return (uint32_t)(s1 % ADLER_MOD); }
MRCNN_PNG_HD uint32_t adler_block_b(unsigned long long s1, unsigned long long s2, long long after)
{
    return (uint32_t)((s2 % ADLER_MOD + (unsigned long long)(after % ADLER_MOD) * (s1 % ADLER_MOD)) % ADLER_MOD);
}
MRCNN_PNG_HD uint32_t adler_fold(unsigned long long sum_a, unsigned long long sum_b, long long n)
{
    const uint32_t a = (uint32_t)((1 + sum_a) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + sum_b) % ADLER_MOD);
    return b << 16 | a;
}

}  // namespace png
}  // namespace mrcnn
