// jpeg_entropy.h — the Huffman decoding step of the self-synchronising entropy stage and one unit's turn around it (its bytes, its
// context, its sink, the writing pass's verdict), written once for both sides: the kernels of kernels_jpeg_entropy.hip and the
// sequential model of jpeg_entropy_host.cpp run these functions.  Plain C++ (g++ builds it alone).
//
// The scan of a file is cut at its markers into SEGMENTS (a restart interval, or the whole scan): each starts on an MCU boundary with
// zeroed predictors.  A segment is cut into UNITS of unit_bytes raw bytes (stuffed zeros included).  A decoder state is
//     (bit position, block inside its MCU, zigzag index)
// with the bit position counted in the file's RAW bytes and never resting on a stuffed zero; inside a segment every FF is followed by
// its stuffed 00, so a 00 behind an FF is always one.  decode_unit() decodes the symbols (a code and its extra bits) that START in a
// unit from a given state; what it calls an anomaly is what jpeg_host.cpp's decode_coefficients refuses: no such code, a DC category
// above 15, a zero run that leaves the block, bits consumed past the end of the segment, a block outside the image.  The one place where
// an anomaly is not one: in the last 7 bits of a segment it only says that those bits are padding and no further block.
#pragma once
#include "jpeg_huff.h"

namespace mrcnn {
namespace jpeg {

constexpr int ENT_UNIT_BYTES = 128;        // production unit
constexpr int ENT_WG_UNITS = 256;          // units (= threads) of a workgroup; a workgroup serves ONE file
constexpr int ENT_SYNC_BYTES = 65536;      // a wrong state may survive this much stream before the file is given to the host decoder
constexpr int ENT_MAX_BPM = 6;             // blocks per MCU of the sampling modes the parser admits (4:2:0)

struct EntFile {
    long long byte0;            // the file's first byte in the batch's byte blob (multiple of 16)
    long long length;
    long long comp_block0[3];   // JpegDesc::comp[c].block0: counted over the whole batch
    int comp_blocks_w[3];
    int seg0, nseg;             // nseg = 0: the marker scan found something the device path leaves to the host decoder
    int unit0, nunits;
    int wg0, nwg;
    int bpm, nluma, hs, vs;     // blocks per MCU; of them luma (hs * vs)
    int mcus_x, mcus_y, ncomp, reserved;
    HuffTable tab[6];           // DC of components 0..2, then AC of components 0..2
};
struct EntSeg {
    long long b0, b1;           // raw bytes [b0, b1) of the file; b1 is the FF of the marker that ends the segment
    long long first_block;      // scan-order number, in its file, of the segment's first block
    int nblocks;                // what the interval must hold
    int file, unit0, nunits;
    int reserved[2];
};
struct EntWg { int file, unit0, count, reserved; };

// status bits of a file (device or model); 0 = clean
enum { ENT_BAD_WRITE = 1,      // an anomaly in the writing pass, or a unit that did not reproduce its recorded state
       ENT_BAD_COUNT = 2,      // an interval with another number of blocks, not ending on an MCU boundary, or 8+ unread bits before its marker
       ENT_BAD_SYNC = 4 };     // a workgroup ran out of rounds

typedef unsigned long long ent_state;
constexpr ent_state ENT_INVALID = ~0ull;
MRCNN_HUFF_HD ent_state ent_pack(long long bitpos, int blk, int zz) { return (ent_state)bitpos | ((ent_state)blk << 32) | ((ent_state)zz << 40); }
MRCNN_HUFF_HD long long ent_pos(ent_state s) { return (long long)(s & 0xFFFFFFFFull); }
MRCNN_HUFF_HD int ent_blk(ent_state s) { return (int)((s >> 32) & 0xFF); }
MRCNN_HUFF_HD int ent_zz(ent_state s) { return (int)((s >> 40) & 0xFF); }

struct EntCtx {
    const uint8_t* data;        // the file's bytes
    const HuffTable* tab;       // EntFile::tab (the kernels: its copy in LDS)
    const uint8_t* zigzag;      // zigzag position -> natural index
    long long b0, b1;           // the segment: raw bytes [b0, b1)
    int bpm, nluma;
};
// where the writing pass puts what it decodes
struct EntSink {
    int16_t* coef;              // the batch's coefficient array
    long long seq0;             // scan-order number (in the file) of the block in progress at the unit's entry state
    long long seq_end;          // first number behind the segment
    long long block0[3];
    int blocks_w[3];
    int hs, vs, mcus_x;
};
struct EntResult {
    ent_state state;            // ENT_INVALID after an anomaly
    int blocks;                 // blocks completed
    int anomaly;
};

// scan-order number -> block of the batch's coefficient array (seq < mcus * bpm: inside the component grids)
MRCNN_HUFF_HD long long ent_block_index(const EntSink& k, long long seq, int bpm, int nluma)
{
    const long long m = seq / bpm;
    const int b = (int)(seq - m * bpm);
    const long long my = m / k.mcus_x, mx = m - my * k.mcus_x;
    if (b < nluma) {
        const int v = b / k.hs, u = b - v * k.hs;
        return k.block0[0] + (my * k.vs + v) * k.blocks_w[0] + mx * k.hs + u;
    }
    return b == nluma ? k.block0[1] + my * k.blocks_w[1] + mx : k.block0[2] + my * k.blocks_w[2] + mx;
}

// the state a unit starts from when nothing better is known: a block starting at its first byte that is not a stuffed zero
MRCNN_HUFF_HD ent_state ent_guess(const uint8_t* data, long long seg_b0, long long unit_b0)
{
    const bool stuffed = unit_b0 > seg_b0 && data[unit_b0 - 1] == 0xFF;
    return ent_pack((unit_b0 + (stuffed ? 1 : 0)) * 8, 0, 0);
}

// DATA bits between position P and the marker that ends segment [b0, b1): the bytes are not unstuffed, so when the segment's last data
// byte is an FF, its stuffed 00 stands in front of the marker and holds no bits (P never rests inside it).
MRCNN_HUFF_HD long long ent_bits_left(const uint8_t* data, long long b0, long long b1, long long P)
{
    const long long raw = b1 * 8 - P;
    if (raw < 8 || raw >= 16) return raw < 0 ? 0 : raw;          // behind the pair (or at the end) | too far to matter
    return b1 - b0 >= 2 && data[b1 - 2] == 0xFF && data[b1 - 1] == 0x00 && P >= (b1 - 2) * 8 ? raw - 8 : raw;
}

// Decodes the symbols that start in raw bytes [unit_b0, unit_b1) of the segment from state `in`; sink != nullptr: writes them (the DC
// as its difference).  Every read is below c.b1; the loop runs once per symbol, at most once per bit of the unit.
MRCNN_HUFF_HD EntResult decode_unit(const EntCtx& c, long long unit_b0, long long unit_b1, ent_state in, const EntSink* sink)
{
    EntResult r;
    r.state = ENT_INVALID; r.blocks = 0; r.anomaly = 1;
    long long P = ent_pos(in);
    int blk = ent_blk(in), zz = ent_zz(in);
    const long long endbits = unit_b1 * 8, segbits = c.b1 * 8;
    // (a state that stopped in front of padding may rest in the FF whose stuffed 00 opens this unit: nothing more starts there, it passes through)
    const long long lo = unit_b0 > c.b0 && c.data[unit_b0 - 1] == 0xFF ? unit_b0 - 1 : unit_b0;
    if (in == ENT_INVALID || P < lo * 8 || P > segbits || blk >= c.bpm || zz > 63 || unit_b1 > c.b1) return r;
    long long seq = sink ? sink->seq0 : 0;
    int16_t* dst = nullptr;
    if (sink && zz > 0) {
        if (seq >= sink->seq_end) return r;
        dst = sink->coef + ent_block_index(*sink, seq, c.bpm, c.nluma) * 64;
    }
    int left = (int)(unit_b1 - unit_b0) * 8 + 1;
    // In front of the marker stand fewer than 8 bits of padding (ones) — or one more short block: DC difference 0 and an end-of-block
    // code are 6 bits with the standard tables, and flat areas end on such blocks.  Which it is, is decided by trying: what decodes to
    // a whole block without leaving the segment is a block; anything else is padding and the state stays in front of it.
    bool trial = false;
    long long trial_P = 0;
    while (P < endbits && left-- > 0) {
        if (zz == 0 && !trial && ent_bits_left(c.data, c.b0, c.b1, P) < 8) { trial = true; trial_P = P; }
        // six data bytes from P's byte on, stuffed zeros skipped, zeros behind the segment
        long long i = P >> 3;
        unsigned long long acc = 0;
        {
            long long j = i;
            for (int k = 0; k < 6; ++k) {
                unsigned b = 0;
                if (j < c.b1) { b = c.data[j]; j += b == 0xFF ? 2 : 1; } else { j += 1; }
                acc = (acc << 8) | b;
            }
        }
        const int sh = (int)(P & 7);
        const uint32_t w = (uint32_t)((acc << (16 + sh)) >> 32);       // the next 32 bits (41 are loaded)
        const int comp = blk < c.nluma ? 0 : blk - c.nluma + 1;
        const HuffTable& t = c.tab[(zz == 0 ? 0 : 3) + comp];
        const int e = huff_lookup(t, w);
        if (!e) { if (trial) goto padding; return r; }                                // no such code
        const int len = e >> 8, sym = e & 255;
        int s, run = 0;
        if (zz == 0) {
            if (sym > 15) { if (trial) goto padding; return r; }                      // DC category
            s = sym;
        } else {
            run = sym >> 4; s = sym & 15;
        }
        int v = 0;
        if (s) {
            const uint32_t x = (uint32_t)(w << len) >> (32 - s);
            v = x < (1u << (s - 1)) ? (int)x - (1 << s) + 1 : (int)x;
        }
        const int o = sh + len + s, nb = o >> 3;         // len + s <= 31: at most four bytes are left behind
        for (int k = 0; k < nb; ++k) i += ((acc >> (40 - 8 * k)) & 0xFF) == 0xFF ? 2 : 1;
        P = i * 8 + (o & 7);
        if (P > segbits) { if (trial) goto padding; return r; }                       // bits consumed past the end of the segment
        if (zz == 0) {
            if (sink) {
                if (seq >= sink->seq_end) { if (trial) goto padding; return r; }      // a block outside the interval
                dst = sink->coef + ent_block_index(*sink, seq, c.bpm, c.nluma) * 64;
                dst[0] = (int16_t)v;
            }
            zz = 1;
        } else if (s) {
            zz += run;
            if (zz > 63) { if (trial) goto padding; return r; }                       // a zero run that leaves the block
            if (sink) dst[c.zigzag[zz]] = (int16_t)v;
            zz += 1;
        } else if (run == 15) {
            zz += 16;
        } else {
            zz = 64;
        }
        if (zz >= 64) {
            zz = 0;
            blk = blk + 1 == c.bpm ? 0 : blk + 1;
            ++r.blocks;
            ++seq;
            trial = false;
        }
    }
    if (trial) {                                         // (the segment ended inside the block on trial)
padding:
        P = trial_P; zz = 0;                             // blk, seq and the count have not moved since the trial began
    }
    r.state = ent_pack(P, blk, zz);
    r.anomaly = 0;
    return r;
}

// One unit's turn, the same on both sides: where it lies, what it decodes with, where it writes, and what the writing pass says of it.
struct EntUnit {
    long long ub, ue;           // raw bytes [ub, ue) of the file
    bool first;                 // of its segment: it starts from the segment's own state, never from a neighbour's
};
MRCNN_HUFF_HD EntUnit ent_unit(const EntSeg& s, int u, int unit_bytes)
{
    EntUnit q;
    q.ub = s.b0 + (long long)(u - s.unit0) * unit_bytes;
    q.ue = q.ub + unit_bytes < s.b1 ? q.ub + unit_bytes : s.b1;
    q.first = u == s.unit0;
    return q;
}

// data: the file's bytes; tab: EntFile::tab or a copy of it.  Two clamps keep a plan that is not plan_entropy's from reading or writing
// outside the file: b1 to the file's length here, seq_end to the MCU grid in ent_write_unit.  Both are no-ops for every plan that
// plan_entropy makes: it accepts a segment only with end + 1 < length, and its segments' nblocks sum to mcus * bpm.
MRCNN_HUFF_HD EntCtx ent_ctx(const EntFile& f, const EntSeg& s, const uint8_t* data, const HuffTable* tab, const uint8_t* zigzag)
{
    EntCtx c;
    c.data = data; c.tab = tab; c.zigzag = zigzag;
    c.b0 = s.b0; c.b1 = s.b1 < f.length ? s.b1 : f.length; c.bpm = f.bpm; c.nluma = f.nluma;
    return c;
}

MRCNN_HUFF_HD EntSink ent_sink(const EntFile& f, int16_t* coef)
{
    EntSink k;
    k.coef = coef; k.seq0 = 0; k.seq_end = 0;
    for (int i = 0; i < 3; ++i) { k.block0[i] = f.comp_block0[i]; k.blocks_w[i] = f.comp_blocks_w[i]; }
    k.hs = f.hs; k.vs = f.vs; k.mcus_x = f.mcus_x;
    return k;
}

// The writing pass of unit u of segment s: decodes it from the state its predecessor recorded into coef (the DC as its difference) and
// returns the status bits.  state: the recorded states, by unit; before / through: the blocks the synchronisation phase counted in the
// segment's units in front of u / up to and including u (their difference is the count recorded for u).
MRCNN_HUFF_HD int ent_write_unit(const EntCtx& c, const EntFile& f, const EntSeg& s, int u, int unit_bytes, const ent_state* state, long long before,
                                 long long through, int16_t* coef)
{
    const EntUnit q = ent_unit(s, u, unit_bytes);
    EntSink k = ent_sink(f, coef);
    const long long mcu_blocks = (long long)f.mcus_x * f.mcus_y * f.bpm;
    k.seq0 = s.first_block + before;
    k.seq_end = s.first_block + s.nblocks < mcu_blocks ? s.first_block + s.nblocks : mcu_blocks;       // (never behind the component grids)
    const EntResult r = decode_unit(c, q.ub, q.ue, q.first ? ent_pack(s.b0 * 8, 0, 0) : state[u - 1], &k);
    int bad = 0;
    if (r.anomaly || r.state != state[u] || r.blocks != through - before) bad |= ENT_BAD_WRITE;
    if (u == s.unit0 + s.nunits - 1) {
        const bool whole = !r.anomaly && ent_zz(r.state) == 0 && ent_blk(r.state) == 0 && ent_bits_left(c.data, c.b0, c.b1, ent_pos(r.state)) < 8 &&
                           through == s.nblocks;
        if (!whole) bad |= ENT_BAD_COUNT;
    }
    return bad;
}

// the launches of the synchronisation phase and the rounds inside one, from the knobs (0 = production)
MRCNN_HUFF_HD int ent_launches(int unit_bytes, int max_file_wgs, int max_rounds)
{
    int n = 2 + (ENT_SYNC_BYTES + ENT_WG_UNITS * unit_bytes - 1) / (ENT_WG_UNITS * unit_bytes);
    if (n > max_file_wgs + 1) n = max_file_wgs + 1;
    if (max_rounds > 0 && n > max_rounds) n = max_rounds;
    return n < 1 ? 1 : n;
}
MRCNN_HUFF_HD int ent_inner_rounds(int max_rounds) { return max_rounds > 0 ? max_rounds : ENT_WG_UNITS + 1; }

}  // namespace jpeg
}  // namespace mrcnn
