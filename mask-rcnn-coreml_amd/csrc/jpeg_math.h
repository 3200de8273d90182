// jpeg_math.h — the per-sample arithmetic of the JPEG decoder, written once for the host definition (jpeg_host.cpp, plain C++) and for
// the kernels (kernels_jpeg.hip): libjpeg's default pipeline — the "islow" inverse DCT, fancy (triangle) chroma upsampling, the 16-bit
// fixed-point YCbCr -> RGB — all in integers, so both sides produce the same bytes by construction.  No HIP header is included here.
// The second half is the encoder's (jpeg_enc_host.cpp, kernels_jpeg_enc.hip): libjpeg's default compressor, shared the same way.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_JPEG_HD __host__ __device__ inline
#else
#define MRCNN_JPEG_HD inline
#endif

namespace mrcnn {
namespace jpeg {

enum { MODE_444 = 0, MODE_H2V1 = 1, MODE_H2V2 = 2 };

// All sums and products run in uint32_t — two's complement wrap-around, defined for ANY coefficient a damaged stream can hold; only
// the descaling shifts are arithmetic.  For encoder-made files nothing wraps and these are libjpeg's numbers.
typedef uint32_t jword;
MRCNN_JPEG_HD jword descale(jword x, int n) { return (jword)((int32_t)(x + ((jword)1 << (n - 1))) >> n); }

enum { CONST_BITS = 13, PASS1_BITS = 2 };
// FIX(x) = round(x * 2^13)
#define MRCNN_JPEG_FIX_0_298631336 2446u
#define MRCNN_JPEG_FIX_0_390180644 3196u
#define MRCNN_JPEG_FIX_0_541196100 4433u
#define MRCNN_JPEG_FIX_0_765366865 6270u
#define MRCNN_JPEG_FIX_0_899976223 7373u
#define MRCNN_JPEG_FIX_1_175875602 9633u
#define MRCNN_JPEG_FIX_1_501321110 12299u
#define MRCNN_JPEG_FIX_1_847759065 15137u
#define MRCNN_JPEG_FIX_1_961570560 16069u
#define MRCNN_JPEG_FIX_2_053119869 16819u
#define MRCNN_JPEG_FIX_2_562915447 20995u
#define MRCNN_JPEG_FIX_3_072711026 25172u

// One 1-D pass of the islow IDCT over eight values, in place.  first = true: the pass over a column of dequantised coefficients
// (descaled by CONST_BITS - PASS1_BITS); false: the pass over a row of the workspace (descaled by CONST_BITS + PASS1_BITS + 3).
MRCNN_JPEG_HD void idct_1d(jword v[8], bool first)
{
    const int shift = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
    // even part
    jword z2 = v[2], z3 = v[6];
    jword z1 = (z2 + z3) * MRCNN_JPEG_FIX_0_541196100;
    jword tmp2 = z1 - z3 * MRCNN_JPEG_FIX_1_847759065;
    jword tmp3 = z1 + z2 * MRCNN_JPEG_FIX_0_765366865;
    z2 = v[0]; z3 = v[4];
    jword tmp0 = (z2 + z3) << CONST_BITS;
    jword tmp1 = (z2 - z3) << CONST_BITS;
    const jword tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    jword z4 = tmp1 + tmp3;
    const jword z5 = (z3 + z4) * MRCNN_JPEG_FIX_1_175875602;
    tmp0 *= MRCNN_JPEG_FIX_0_298631336;
    tmp1 *= MRCNN_JPEG_FIX_2_053119869;
    tmp2 *= MRCNN_JPEG_FIX_3_072711026;
    tmp3 *= MRCNN_JPEG_FIX_1_501321110;
    z1 = (jword)0 - z1 * MRCNN_JPEG_FIX_0_899976223;
    z2 = (jword)0 - z2 * MRCNN_JPEG_FIX_2_562915447;
    z3 = (jword)0 - z3 * MRCNN_JPEG_FIX_1_961570560;
    z4 = (jword)0 - z4 * MRCNN_JPEG_FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    v[0] = descale(tmp10 + tmp3, shift); v[7] = descale(tmp10 - tmp3, shift);
    v[1] = descale(tmp11 + tmp2, shift); v[6] = descale(tmp11 - tmp2, shift);
    v[2] = descale(tmp12 + tmp1, shift); v[5] = descale(tmp12 - tmp1, shift);
    v[3] = descale(tmp13 + tmp0, shift); v[4] = descale(tmp13 - tmp0, shift);
}

MRCNN_JPEG_HD uint8_t clamp_u8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// a row pass's result -> sample: + 128, clamped
MRCNN_JPEG_HD uint8_t idct_sample(jword v) { return clamp_u8((int32_t)v + 128); }

// One chroma sample at output pixel (x, y), from the component's own plane of cw x ch REAL samples (row pitch `pitch`; what the
// padding of the block grid holds beyond them is never read).  libjpeg picks the triangle filter only where the plane is more than
// two samples wide; narrower planes are replicated.
MRCNN_JPEG_HD int32_t chroma_at(const uint8_t* plane, int64_t pitch, int cw, int ch, int x, int y, int mode)
{
    if (mode == MODE_444) return plane[(int64_t)y * pitch + x];
    const int cx = x >> 1;
    if (mode == MODE_H2V1) {
        const uint8_t* row = plane + (int64_t)y * pitch;
        const int32_t c = row[cx];
        if (cw <= 2) return c;
        if (x & 1) return cx == cw - 1 ? c : (3 * c + row[cx + 1] + 2) >> 2;
        return cx == 0 ? c : (3 * c + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = plane + (int64_t)cy * pitch;
    if (cw <= 2) return near[cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;                 // the row above for even output rows, below for odd ones; replicated at the ends
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const uint8_t* far = plane + (int64_t)fy * pitch;
    const int32_t s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

// -> R | G << 8 | B << 16
MRCNN_JPEG_HD uint32_t ycc_to_rgb(int32_t y, int32_t cb, int32_t cr)
{
    cb -= 128; cr -= 128;
    return (uint32_t)clamp_u8(y + ((91881 * cr + 32768) >> 16)) | (uint32_t)clamp_u8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16)) << 8 |
           (uint32_t)clamp_u8(y + ((116130 * cb + 32768) >> 16)) << 16;
}

// Sample planes of one image: plane[c] has pitch[c] bytes per row; chroma planes hold cw x ch real samples.
struct Planes {
    const uint8_t* plane[3];
    int64_t pitch[3];
    int ncomp, mode, cw, ch;
};
// the pixel at (x, y) as R | G << 8 | B << 16
MRCNN_JPEG_HD uint32_t pixel_rgb(const Planes& p, int x, int y)
{
    const int32_t yy = p.plane[0][(int64_t)y * p.pitch[0] + x];
    if (p.ncomp == 1) return (uint32_t)yy * 0x010101u;
    return ycc_to_rgb(yy, chroma_at(p.plane[1], p.pitch[1], p.cw, p.ch, x, y, p.mode), chroma_at(p.plane[2], p.pitch[2], p.cw, p.ch, x, y, p.mode));
}

// ================================================================================================
// The forward path (jpeg_enc_host.cpp, kernels_jpeg_enc.hip): libjpeg's default compressor in integers — 16-bit fixed-point
// RGB -> YCbCr, box chroma downsampling with the alternating bias, edge replication, the "islow" forward DCT, division by 8q.
// Samples are 0..255, so nothing here leaves int32.
// ================================================================================================
enum { ENC_444 = 0, ENC_422 = 1, ENC_420 = 2, ENC_GREY = 3 };      // = MRCNN_JPEG_444 ..

MRCNN_JPEG_HD int32_t rgb_to_y(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
MRCNN_JPEG_HD int32_t rgb_to_cb(int32_t r, int32_t g, int32_t b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
MRCNN_JPEG_HD int32_t rgb_to_cr(int32_t r, int32_t g, int32_t b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// component c (0 = Y, 1 = Cb, 2 = Cr) of the pixel at (x, y), both clamped into the image: the edge replication
MRCNN_JPEG_HD int32_t enc_pixel(const uint8_t* rgb, int h, int w, int c, int x, int y)
{
    x = x < w - 1 ? x : w - 1;
    y = y < h - 1 ? y : h - 1;
    const uint8_t* p = rgb + ((int64_t)y * w + x) * 3;
    return c == 0 ? rgb_to_y(p[0], p[1], p[2]) : (c == 1 ? rgb_to_cb(p[0], p[1], p[2]) : rgb_to_cr(p[0], p[1], p[2]));
}

// sample (sx, sy) of component c on its own (downsampled) grid, any sx, sy >= 0: the bias of a chroma box alternates along a row,
// 0,1,.. for two samples (h2v1) and 1,2,.. for four (h2v2)
MRCNN_JPEG_HD int32_t enc_sample(const uint8_t* rgb, int h, int w, int sampling, int c, int sx, int sy)
{
    if (c == 0 || sampling == ENC_444 || sampling == ENC_GREY) return enc_pixel(rgb, h, w, c, sx, sy);
    if (sampling == ENC_422) return (enc_pixel(rgb, h, w, c, 2 * sx, sy) + enc_pixel(rgb, h, w, c, 2 * sx + 1, sy) + (sx & 1)) >> 1;
    // libjpeg replicates columns BEFORE downsampling but rows of a component AFTER it: below the image a chroma row repeats the last
    // real chroma row (rows h-2 and h-1 when h is even), which clamping the two source rows alone would not give
    const int last = (h + 1) / 2 - 1;
    sy = sy < last ? sy : last;
    return (enc_pixel(rgb, h, w, c, 2 * sx, 2 * sy) + enc_pixel(rgb, h, w, c, 2 * sx + 1, 2 * sy) + enc_pixel(rgb, h, w, c, 2 * sx, 2 * sy + 1) +
            enc_pixel(rgb, h, w, c, 2 * sx + 1, 2 * sy + 1) + 1 + (sx & 1)) >> 2;
}

MRCNN_JPEG_HD int32_t fdescale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of jfdctint over eight values, in place.  first = true: the pass over a row of level-shifted samples (results scaled
// up by 2^PASS1_BITS); false: the pass over a column of the workspace (that scaling removed; the output stays 8x the true DCT).
MRCNN_JPEG_HD void fdct_1d(int32_t v[8], bool first)
{
    int32_t tmp0 = v[0] + v[7], tmp7 = v[0] - v[7], tmp1 = v[1] + v[6], tmp6 = v[1] - v[6];
    int32_t tmp2 = v[2] + v[5], tmp5 = v[2] - v[5], tmp3 = v[3] + v[4], tmp4 = v[3] - v[4];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int shift = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if (first) {
        v[0] = (tmp10 + tmp11) * (1 << PASS1_BITS);
        v[4] = (tmp10 - tmp11) * (1 << PASS1_BITS);
    } else {
        v[0] = fdescale(tmp10 + tmp11, PASS1_BITS);
        v[4] = fdescale(tmp10 - tmp11, PASS1_BITS);
    }
    int32_t z1 = (tmp12 + tmp13) * (int32_t)MRCNN_JPEG_FIX_0_541196100;
    v[2] = fdescale(z1 + tmp13 * (int32_t)MRCNN_JPEG_FIX_0_765366865, shift);
    v[6] = fdescale(z1 - tmp12 * (int32_t)MRCNN_JPEG_FIX_1_847759065, shift);
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * (int32_t)MRCNN_JPEG_FIX_1_175875602;
    tmp4 *= (int32_t)MRCNN_JPEG_FIX_0_298631336;
    tmp5 *= (int32_t)MRCNN_JPEG_FIX_2_053119869;
    tmp6 *= (int32_t)MRCNN_JPEG_FIX_3_072711026;
    tmp7 *= (int32_t)MRCNN_JPEG_FIX_1_501321110;
    z1 *= -(int32_t)MRCNN_JPEG_FIX_0_899976223;
    z2 *= -(int32_t)MRCNN_JPEG_FIX_2_562915447;
    z3 *= -(int32_t)MRCNN_JPEG_FIX_1_961570560;
    z4 *= -(int32_t)MRCNN_JPEG_FIX_0_390180644;
    z3 += z5; z4 += z5;
    v[7] = fdescale(tmp4 + z1 + z3, shift);
    v[5] = fdescale(tmp5 + z2 + z4, shift);
    v[3] = fdescale(tmp6 + z2 + z3, shift);
    v[1] = fdescale(tmp7 + z1 + z4, shift);
}

// a DCT output (8x scaled) over quantiser q: division by 8q, halves rounded away from zero
MRCNN_JPEG_HD int32_t quantise(int32_t v, int32_t q)
{
    const int32_t d = q << 3;
    return v < 0 ? -((-v + (d >> 1)) / d) : (v + (d >> 1)) / d;
}

// ---- entropy coding of one coefficient: what it appends to the scan, as (bits, their count) ----
struct Code { uint64_t bits; int len; };              // len <= 59, the bits right-aligned

MRCNN_JPEG_HD int size_category(int32_t v)            // bits of |v|: 0 for 0, 11 at most (a DC difference)
{
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}
MRCNN_JPEG_HD void code_append(Code& c, uint32_t bits, int len) { c.bits = (c.bits << len) | bits; c.len += len; }

// A Huffman table as the encoder reads it: entry[symbol] = length << 16 | code.  dc: 12 symbols; ac: 256 (run << 4 | size).
// The DC difference `diff` of a block: its size's code, then the size's low bits of diff (of diff - 1 when negative).
MRCNN_JPEG_HD Code code_dc(const uint32_t* dc, int32_t diff)
{
    Code c = {0, 0};
    const int s = size_category(diff);
    code_append(c, dc[s] & 0xFFFFu, (int)(dc[s] >> 16));
    if (s) code_append(c, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    return c;
}
// A non-zero AC coefficient v after `run` zeros (0..62): run / 16 ZRL codes, the code of (run % 16, size), the size's low bits.
MRCNN_JPEG_HD Code code_ac(const uint32_t* ac, int run, int32_t v)
{
    Code c = {0, 0};
    for (int i = run >> 4; i > 0; --i) code_append(c, ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
    const int s = size_category(v), sym = ((run & 15) << 4) | s;
    code_append(c, ac[sym] & 0xFFFFu, (int)(ac[sym] >> 16));
    code_append(c, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
    return c;
}
MRCNN_JPEG_HD Code code_eob(const uint32_t* ac) { Code c = {ac[0] & 0xFFFFu, (int)(ac[0] >> 16)}; return c; }

}  // namespace jpeg
}  // namespace mrcnn
