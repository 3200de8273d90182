// jpeg_host.cpp — see jpeg_host.h.  Plain C++17, no HIP.
#include "jpeg_host.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "jpeg_math.h"

namespace mrcnn {
namespace jpeg {

namespace {

int fail(std::string* err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(std::string* err, int code, const char* fmt, ...)
{
    if (err) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        *err = buf;
    }
    return code;
}

const char* sof_name(int m)
{
    switch (m) {
    case 0xC1: return "extended sequential DCT (SOF1)";
    case 0xC2: return "progressive DCT (SOF2)";
    case 0xC3: return "lossless (SOF3)";
    case 0xC5: return "differential sequential DCT (SOF5)";
    case 0xC6: return "differential progressive DCT (SOF6)";
    case 0xC7: return "differential lossless (SOF7)";
    case 0xC9: return "arithmetic-coded sequential DCT (SOF9)";
    case 0xCA: return "arithmetic-coded progressive DCT (SOF10)";
    case 0xCB: return "arithmetic-coded lossless (SOF11)";
    case 0xCD: return "arithmetic-coded differential sequential DCT (SOF13)";
    case 0xCE: return "arithmetic-coded differential progressive DCT (SOF14)";
    default: return "arithmetic-coded differential lossless (SOF15)";
    }
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

}  // namespace

int parse(const uint8_t* data, int64_t length, Header* out, std::string* err)
{
    if (!out || length < 0 || (!data && length > 0)) return fail(err, MRCNN_ERR_INVALID, "jpeg: null data or negative length");
    Header& h = *out;
    memset(&h, 0, sizeof h);
    if (length < 2 || data[0] != 0xFF || data[1] != 0xD8) return fail(err, MRCNN_ERR_IO, "jpeg: the data does not start with SOI (FF D8)");
    int64_t pos = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    for (;;) {
        if (pos + 2 > length) return fail(err, MRCNN_ERR_IO, "jpeg: truncated before the scan (at byte %lld)", (long long)pos);
        if (data[pos] != 0xFF) return fail(err, MRCNN_ERR_IO, "jpeg: expected a marker at byte %lld, found %02X", (long long)pos, data[pos]);
        while (pos + 1 < length && data[pos + 1] == 0xFF) ++pos;          // fill bytes
        if (pos + 2 > length) return fail(err, MRCNN_ERR_IO, "jpeg: truncated inside a marker");
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD9))
            return fail(err, MRCNN_ERR_IO, "jpeg: marker FF %02X before the scan", m);
        if (pos + 2 > length) return fail(err, MRCNN_ERR_IO, "jpeg: truncated inside segment FF %02X", m);
        const int L = be16(data + pos);
        if (L < 2 || pos + L > length) return fail(err, MRCNN_ERR_IO, "jpeg: segment FF %02X of length %d is truncated or malformed", m, L);
        const uint8_t* s = data + pos + 2;
        const int n = L - 2;
        pos += L;
        if (m == 0xC0) {
            if (have_sof) return fail(err, MRCNN_ERR_IO, "jpeg: a second frame header");
            if (n < 6) return fail(err, MRCNN_ERR_IO, "jpeg: short SOF0 segment");
            const int precision = s[0], nc = s[5];
            h.height = be16(s + 1);
            h.width = be16(s + 3);
            if (precision != 8) return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: %d-bit samples (only 8-bit baseline is decoded)", precision);
            if (nc != 1 && nc != 3) return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: %d components (only 1 = grey and 3 = YCbCr are decoded)", nc);
            if (n != 6 + 3 * nc) return fail(err, MRCNN_ERR_IO, "jpeg: SOF0 length does not match its %d components", nc);
            if (h.height == 0) return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: height 0 (a DNL-defined height is not decoded)");
            if (h.width == 0) return fail(err, MRCNN_ERR_IO, "jpeg: width 0");
            if (h.height > 32767 || h.width > 32767)
                return fail(err, MRCNN_ERR_SHAPE, "jpeg: the image is %dx%d: height and width must lie in 1..32767", h.height, h.width);
            h.components = nc;
            for (int c = 0; c < nc; ++c) {
                Component& k = h.comp[c];
                k.id = s[6 + 3 * c];
                k.h_samp = s[7 + 3 * c] >> 4;
                k.v_samp = s[7 + 3 * c] & 15;
                k.tq = s[8 + 3 * c];
                if (k.h_samp < 1 || k.h_samp > 4 || k.v_samp < 1 || k.v_samp > 4 || k.tq > 3)
                    return fail(err, MRCNN_ERR_IO, "jpeg: component %d has sampling %dx%d, table %d", c, k.h_samp, k.v_samp, k.tq);
            }
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: %s (only baseline SOF0 is decoded)", sof_name(m));
        } else if (m == 0xC8) {
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: JPEG extension frame (FF C8)");
        } else if (m == 0xCC) {
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: arithmetic conditioning table (DAC): arithmetic coding is not decoded");
        } else if (m == 0xDC) {
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: DNL marker");
        } else if (m == 0xDB) {
            int i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3) return fail(err, MRCNN_ERR_IO, "jpeg: DQT with precision %d, table %d", pq, tq);
                const int need = 1 + 64 * (pq + 1);
                if (i + need > n) return fail(err, MRCNN_ERR_IO, "jpeg: truncated DQT");
                for (int k = 0; k < 64; ++k)
                    h.quant[tq][kZigzag[k]] = (uint16_t)(pq ? be16(s + i + 1 + 2 * k) : s[i + 1 + k]);
                h.quant_defined[tq] = true;
                i += need;
            }
        } else if (m == 0xC4) {
            int i = 0;
            while (i < n) {
                if (i + 17 > n) return fail(err, MRCNN_ERR_IO, "jpeg: truncated DHT");
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return fail(err, MRCNN_ERR_IO, "jpeg: DHT with class %d, table %d", tc, th);
                HuffSpec& t = tc ? h.ac[th] : h.dc[th];
                t.bits[0] = 0;
                int count = 0;
                for (int l = 1; l <= 16; ++l) { t.bits[l] = s[i + l]; count += s[i + l]; }
                if (count > 256 || i + 17 + count > n) return fail(err, MRCNN_ERR_IO, "jpeg: DHT with %d symbols is truncated or malformed", count);
                // the codes must fit their lengths (Kraft): a table that does not is refused here, once
                unsigned code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += t.bits[l];
                    if (code > (1u << l)) return fail(err, MRCNN_ERR_IO, "jpeg: DHT assigns more codes of length %d than exist", l);
                    code <<= 1;
                }
                memset(t.vals, 0, sizeof t.vals);
                memcpy(t.vals, s + i + 17, (size_t)count);
                t.count = count;
                t.defined = true;
                i += 17 + count;
            }
        } else if (m == 0xDD) {
            if (n != 2) return fail(err, MRCNN_ERR_IO, "jpeg: DRI of length %d", L);
            h.restart_interval = be16(s);
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return fail(err, MRCNN_ERR_IO, "jpeg: a scan before the frame header");
            if (n < 1) return fail(err, MRCNN_ERR_IO, "jpeg: short SOS");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return fail(err, MRCNN_ERR_IO, "jpeg: SOS of %d components, length %d", ns, L);
            if (ns != h.components)
                return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: a scan of %d of the frame's %d components (multi-scan sequential files are not decoded)",
                            ns, h.components);
            for (int c = 0; c < ns; ++c) {
                Component& k = h.comp[c];
                if (s[1 + 2 * c] != k.id)
                    return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: the scan lists its components in another order than the frame");
                k.td = s[2 + 2 * c] >> 4;
                k.ta = s[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3 || !h.dc[k.td].defined || !h.ac[k.ta].defined)
                    return fail(err, MRCNN_ERR_IO, "jpeg: component %d uses Huffman tables %d/%d that the file does not define", c, k.td, k.ta);
                if (!h.quant_defined[k.tq]) return fail(err, MRCNN_ERR_IO, "jpeg: component %d uses quantisation table %d that the file does not define", c, k.tq);
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahal != 0) return fail(err, MRCNN_ERR_IO, "jpeg: a baseline scan with Ss=%d Se=%d AhAl=%02X", ss, se, ahal);
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
    // colour space, the way libjpeg guesses it
    if (h.components == 3) {
        if (adobe && !jfif && adobe_transform != 1)
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: Adobe colour transform %d (only YCbCr = 1 is decoded)", adobe_transform);
        if (!adobe && !jfif && h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B')
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: components named R, G, B (only YCbCr is decoded)");
    }
    // sampling
    if (h.components == 1) {
        h.comp[0].h_samp = h.comp[0].v_samp = 1;            // a one-component scan is never interleaved: the factors do not matter
        h.mode = MODE_444;
    } else {
        const Component* k = h.comp;
        const bool chroma_1x1 = k[1].h_samp == 1 && k[1].v_samp == 1 && k[2].h_samp == 1 && k[2].v_samp == 1;
        if (chroma_1x1 && k[0].h_samp == 1 && k[0].v_samp == 1) h.mode = MODE_444;
        else if (chroma_1x1 && k[0].h_samp == 2 && k[0].v_samp == 1) h.mode = MODE_H2V1;
        else if (chroma_1x1 && k[0].h_samp == 2 && k[0].v_samp == 2) h.mode = MODE_H2V2;
        else
            return fail(err, MRCNN_ERR_UNSUPPORTED, "jpeg: sampling factors %dx%d,%dx%d,%dx%d (only 4:4:4, 4:2:2 = 2x1,1x1,1x1 and 4:2:0 = 2x2,1x1,1x1 are decoded)",
                        k[0].h_samp, k[0].v_samp, k[1].h_samp, k[1].v_samp, k[2].h_samp, k[2].v_samp);
    }
    h.h_samp = h.comp[0].h_samp;
    h.v_samp = h.comp[0].v_samp;
    h.mcus_x = (h.width + 8 * h.h_samp - 1) / (8 * h.h_samp);
    h.mcus_y = (h.height + 8 * h.v_samp - 1) / (8 * h.v_samp);
    int64_t at = 0;
    for (int c = 0; c < h.components; ++c) {
        Component& k = h.comp[c];
        k.width = (h.width * k.h_samp + h.h_samp - 1) / h.h_samp;
        k.height = (h.height * k.v_samp + h.v_samp - 1) / h.v_samp;
        k.blocks_w = h.mcus_x * k.h_samp;
        k.blocks_h = h.mcus_y * k.v_samp;
        k.block0 = at;
        at += (int64_t)k.blocks_w * k.blocks_h;
    }
    h.total_blocks = at;
    h.scan_offset = pos;
    // a block costs at least two bits (one DC code, one end-of-block code): a frame size the scan cannot possibly fill is refused before
    // anything is sized by it
    if ((length - pos) * 8 < h.total_blocks * 2)
        return fail(err, MRCNN_ERR_IO, "jpeg: truncated: %lld bytes of scan data cannot hold the %lld blocks of a %dx%d frame", (long long)(length - pos),
                    (long long)h.total_blocks, h.height, h.width);
    return MRCNN_OK;
}

void build_huff_table(const HuffSpec& s, HuffTable& t)
{
    memset(&t, 0, sizeof t);
    memcpy(t.vals, s.vals, sizeof t.vals);
    t.count = s.count;
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        for (int i = 0; i < s.bits[l]; ++i, ++k, ++code) {
            if (l <= 9) {
                const int first = code << (9 - l), span = 1 << (9 - l);
                for (int j = 0; j < span; ++j) t.look[first + j] = (uint16_t)((l << 8) | s.vals[k]);
            }
        }
        t.maxcode[l] = s.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
}

namespace {

// MSB-first bit reader over the entropy-coded segment.  It stops at the first marker (or at the end of the data) and supplies zero
// bits from there on, counting them: consuming one of those is the error `overrun`, checked by the caller once per block.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf = 0;
    int count = 0, pad = 0;
    bool stopped = false, overrun = false;

    void fill()
    {
        while (count <= 56) {
            if (!stopped) {
                if (p >= end) { stopped = true; continue; }
                const uint8_t b = *p;
                if (b == 0xFF) {
                    if (p + 1 < end && p[1] == 0x00) p += 2;         // a stuffed FF
                    else { stopped = true; continue; }              // a marker (p stays on its FF), or the data ends inside one
                } else {
                    ++p;
                }
                buf |= (uint64_t)b << (56 - count);
                count += 8;
            } else {
                count += 8;
                pad += 8;
            }
        }
    }
    int peek(int n) const { return (int)(buf >> (64 - n)); }     // 1 <= n <= 16, after fill()
    void consume(int n)
    {
        buf <<= n;
        count -= n;
        if (count < pad) overrun = true;
    }
    void reset() { buf = 0; count = 0; pad = 0; stopped = false; }
};

// -1: no such code
inline int decode_symbol(BitReader& br, const HuffTable& t)
{
    br.fill();
    const int e = huff_lookup(t, (uint32_t)(br.buf >> 32));
    if (!e) return -1;
    br.consume(e >> 8);
    return e & 255;
}

inline int receive_extend(BitReader& br, int s)     // 1 <= s <= 15
{
    br.fill();
    const int v = br.peek(s);
    br.consume(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// after the bits of an interval: the marker that must follow.  Returns its second byte, -1 when there is none.
int next_marker(BitReader& br)
{
    const uint8_t* p = br.p;
    if (p >= br.end || *p != 0xFF) return -1;
    while (p + 1 < br.end && p[1] == 0xFF) ++p;
    if (p + 1 >= br.end) return -1;
    br.p = p + 2;
    return p[1];
}

}  // namespace

int decode_coefficients(const uint8_t* data, int64_t length, const Header& h, int16_t* coef, std::string* err)
{
    if (!data || !coef) return fail(err, MRCNN_ERR_INVALID, "jpeg: null buffer");
    if (h.scan_offset < 0 || h.scan_offset > length) return fail(err, MRCNN_ERR_INVALID, "jpeg: the header does not belong to this data");
    memset(coef, 0, (size_t)h.total_blocks * 64 * sizeof(int16_t));
    HuffTable dc[4], ac[4];
    for (int i = 0; i < 4; ++i) {
        if (h.dc[i].defined) build_huff_table(h.dc[i], dc[i]);
        if (h.ac[i].defined) build_huff_table(h.ac[i], ac[i]);
    }
    BitReader br;
    br.p = data + h.scan_offset;
    br.end = data + length;
    int pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)h.mcus_x * h.mcus_y;
    int64_t until_restart = h.restart_interval ? h.restart_interval : -1;
    int next_rst = 0;
    int64_t m = 0;
    for (int my = 0; my < h.mcus_y; ++my) {
        for (int mx = 0; mx < h.mcus_x; ++mx, ++m) {
            if (until_restart == 0) {
                br.reset();
                const int got = next_marker(br);
                if (got != 0xD0 + next_rst)
                    return fail(err, MRCNN_ERR_IO, "jpeg: damaged stream: restart marker RST%d expected before MCU %lld", next_rst, (long long)m);
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                until_restart = h.restart_interval;
            }
            for (int c = 0; c < h.components; ++c) {
                const Component& k = h.comp[c];
                const HuffTable& tdc = dc[k.td];
                const HuffTable& tac = ac[k.ta];
                for (int v = 0; v < k.v_samp; ++v) {
                    for (int u = 0; u < k.h_samp; ++u) {
                        int16_t* blk = coef + (k.block0 + (int64_t)(my * k.v_samp + v) * k.blocks_w + (mx * k.h_samp + u)) * 64;
                        int s = decode_symbol(br, tdc);
                        if (s < 0 || s > 15) return fail(err, MRCNN_ERR_IO, "jpeg: damaged stream: bad DC code in MCU %lld", (long long)m);
                        const int diff = s ? receive_extend(br, s) : 0;
                        pred[c] = (int16_t)(uint16_t)(uint32_t)(pred[c] + diff);        // (wraps like the int16 it is stored in)
                        blk[0] = (int16_t)pred[c];
                        for (int i = 1; i < 64; ++i) {
                            const int rs = decode_symbol(br, tac);
                            if (rs < 0) return fail(err, MRCNN_ERR_IO, "jpeg: damaged stream: bad AC code in MCU %lld", (long long)m);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s) {
                                i += r;
                                if (i > 63) return fail(err, MRCNN_ERR_IO, "jpeg: damaged stream: a zero run leaves the block in MCU %lld", (long long)m);
                                blk[kZigzag[i]] = (int16_t)receive_extend(br, s);
                            } else if (r == 15) {
                                i += 15;
                            } else {
                                break;
                            }
                        }
                        if (br.overrun)
                            return fail(err, MRCNN_ERR_IO, "jpeg: truncated or damaged stream: the scan data ends inside MCU %lld of %lld", (long long)m,
                                        (long long)mcus);
                    }
                }
            }
            if (until_restart > 0) --until_restart;
        }
    }
    br.reset();
    if (next_marker(br) != 0xD9) return fail(err, MRCNN_ERR_IO, "jpeg: truncated or damaged stream: no EOI after the scan");
    return MRCNN_OK;
}

// dequantise + both IDCT passes of one block -> 8 rows of 8 samples at out (row pitch `pitch`)
static void idct_block(const int16_t* blk, const uint16_t* q, uint8_t* out, int64_t pitch)
{
    jword ws[64];
    for (int i = 0; i < 64; ++i) ws[i] = (jword)(int32_t)blk[i] * (jword)q[i];
    for (int c = 0; c < 8; ++c) {
        jword v[8];
        for (int r = 0; r < 8; ++r) v[r] = ws[r * 8 + c];
        idct_1d(v, true);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = v[r];
    }
    for (int r = 0; r < 8; ++r) {
        idct_1d(ws + r * 8, false);
        for (int c = 0; c < 8; ++c) out[r * pitch + c] = idct_sample(ws[r * 8 + c]);
    }
}

int decode_host(const uint8_t* data, int64_t length, uint8_t* rgb, int64_t capacity, std::string* err)
{
    Header h;
    int st = parse(data, length, &h, err);
    if (st != MRCNN_OK) return st;
    if (!rgb) return fail(err, MRCNN_ERR_INVALID, "jpeg: null rgb buffer");
    const int64_t need = (int64_t)h.height * h.width * 3;
    if (capacity < need)
        return fail(err, MRCNN_ERR_SHAPE, "jpeg: the %dx%d image needs %lld bytes, the buffer holds %lld", h.height, h.width, (long long)need, (long long)capacity);
    try {
        std::vector<int16_t> coef((size_t)h.total_blocks * 64);
        st = decode_coefficients(data, length, h, coef.data(), err);
        if (st != MRCNN_OK) return st;
        std::vector<uint8_t> planes[3];
        Planes p;
        p.ncomp = h.components; p.mode = h.mode;
        p.cw = h.comp[h.components - 1].width; p.ch = h.comp[h.components - 1].height;
        for (int c = 0; c < h.components; ++c) {
            const Component& k = h.comp[c];
            const int64_t pitch = (int64_t)k.blocks_w * 8;
            planes[c].resize((size_t)(pitch * k.blocks_h * 8));
            for (int by = 0; by < k.blocks_h; ++by)
                for (int bx = 0; bx < k.blocks_w; ++bx)
                    idct_block(coef.data() + (k.block0 + (int64_t)by * k.blocks_w + bx) * 64, h.quant[k.tq], planes[c].data() + (int64_t)by * 8 * pitch + bx * 8, pitch);
            p.plane[c] = planes[c].data();
            p.pitch[c] = pitch;
        }
        for (int y = 0; y < h.height; ++y)
            for (int x = 0; x < h.width; ++x) {
                const uint32_t v = pixel_rgb(p, x, y);
                uint8_t* o = rgb + ((int64_t)y * h.width + x) * 3;
                o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
            }
    } catch (const std::bad_alloc&) {
        return fail(err, MRCNN_ERR_INVALID, "jpeg: out of memory decoding a %dx%d image", h.height, h.width);
    }
    return MRCNN_OK;
}

}  // namespace jpeg
}  // namespace mrcnn
