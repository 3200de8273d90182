// kernels_png.hip — a PNG encoder for a ragged batch of label images (uint8 planes, int16 instance maps), the deflate stream made on
// the device (mrcnn_png_encode_batch); two fills and four launches whatever the batch:
//   k_png_count   one workgroup per deflate block (4096 raw bytes): the bits its tokens take, and its share of the image's Adler-32
//   k_png_scan    exclusive scan of those (one block) + the lengths and offsets of the finished files
//   k_png_pack    the same walk: every lane ORs its token into the zeroed files, addressed by bit position in the whole buffer
//   k_png_frame   the chunks built on the host, IDAT's length and type, the zlib header, the Adler-32 and IEND
// IDAT's CRC-32 is NOT computed here: the files are host memory by contract and a label file is a few KB, so api_png.hip fills it in
// with a table after the copy (no codec is linked).
//
// The format, the token at a position and its bits are png_format.h's — the inline functions the host definition (png_host.cpp) runs
// — so the files equal mrcnn_png_encode_host's byte for byte.  The host parses greedily; here the rule's closed form is used: a
// position needs only the ends of the run of "equal to the byte before" it lies in, found from a 64 x 64-bit mask of the block with
// one forward and one backward scan.  Deflate's bit order is least significant first, so a little-endian word stream is the byte
// stream.  Plain HIP C++, vector stores and vector atomics only; every loop is bounded by a kernel argument (a size read from device
// memory is clamped to one).
#include "kernels.h"
#include "png_format.h"
#include "scan_device.h"

namespace mrcnn {

namespace {

constexpr int PNG_THREADS = 1024;                       // 16 waves; thread t has positions t, t + 1024, t + 2048, t + 3072 of the block
constexpr int PNG_ROUNDS = png::PNG_BLOCK_BYTES / PNG_THREADS;
constexpr int PNG_WORDS = png::PNG_BLOCK_BYTES / 64;    // round r of wave v covers positions [64 k, 64 k + 64), k = 16 r + v
static_assert(PNG_WORDS == 64 && PNG_ROUNDS * (PNG_THREADS / 64) == PNG_WORDS, "one wave scans the block's words, a lane each");

struct PngShared {
    uint8_t raw[png::PNG_BLOCK_BYTES + 16];             // raw[0]: the byte before the block; raw[1 + i]: R[b0 + i]
    unsigned long long equal[PNG_WORDS];                // bit j of word k: R[b0 + 64 k + j] equals the byte before it
    int last_break[PNG_WORDS];                          // the last position of words 0..k that is not equal (-1: none)
    int next_break[PNG_WORDS];                          // the first position of words k..63 that is not equal (4096: none)
    uint32_t word_bits[PNG_WORDS], word_base[PNG_WORDS];
    uint32_t total_bits;
    unsigned long long sums[2][PNG_THREADS / 64];
};

// what a thread holds of its block after the walk
struct PngWalk {
    png::Token token[PNG_ROUNDS];                       // the token that starts at its position of round r (len 0: none)
    uint32_t at[PNG_ROUNDS];                            // its first bit, counted from the block's first
    uint32_t byte[PNG_ROUNDS];
    int len;                                            // raw bytes in the block
};

// Every thread of the workgroup calls it for block `local` of image d.  sh.total_bits = header + tokens + end of block.
__device__ inline void png_walk(const PngDesc& d, long long local, int format, int rows, PngShared& sh, PngWalk& k)
{
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long b0 = local * png::PNG_BLOCK_BYTES;
    const long long left = d.n - b0;
    k.len = (int)(left < png::PNG_BLOCK_BYTES ? (left > 0 ? left : 0) : png::PNG_BLOCK_BYTES);
#pragma unroll
    for (int r = 0; r < PNG_ROUNDS; ++r) {
        const int i = r * PNG_THREADS + t;
        sh.raw[1 + i] = (uint8_t)(i < k.len ? png::raw_byte(d.pixels, d.w, b0 + i, format, rows) : 0u);
    }
    if (t == 0) sh.raw[0] = (uint8_t)(b0 > 0 && k.len > 0 ? png::raw_byte(d.pixels, d.w, b0 - 1, format, rows) : 0u);
    __syncthreads();
    bool equal[PNG_ROUNDS];
#pragma unroll
    for (int r = 0; r < PNG_ROUNDS; ++r) {
        const int i = r * PNG_THREADS + t;
        k.byte[r] = sh.raw[1 + i];
        equal[r] = i < k.len && b0 + i > 0 && sh.raw[1 + i] == sh.raw[i];
        const unsigned long long word = __ballot(equal[r]);
        if (lane == 0) sh.equal[r * (PNG_THREADS / 64) + wave] = word;
    }
    __syncthreads();
    if (wave == 0) {                                    // lane = word: the forward and the backward scan over the breaks
        const unsigned long long breaks = ~sh.equal[lane];
        int last = breaks ? lane * 64 + 63 - __clzll((long long)breaks) : -1;
        int next = breaks ? lane * 64 + __ffsll(breaks) - 1 : (int)png::PNG_BLOCK_BYTES;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int before = __shfl_up(last, s), after = __shfl_down(next, s);
            if (lane >= s && before > last) last = before;
            if (lane + s < 64 && after < next) next = after;
        }
        sh.last_break[lane] = last;
        sh.next_break[lane] = next;
    }
    __syncthreads();
    int upto[PNG_ROUNDS];
#pragma unroll
    for (int r = 0; r < PNG_ROUNDS; ++r) {
        const int i = r * PNG_THREADS + t, word = r * (PNG_THREADS / 64) + wave;
        int kind = i < k.len ? 1 : 0;                   // 0 nothing starts here, 1 a literal, >= 3 a match of that length
        if (equal[r]) {
            const unsigned long long breaks = ~sh.equal[word];
            const unsigned long long below = breaks & ((1ull << lane) - 1), above = lane < 63 ? breaks & ~((2ull << lane) - 1) : 0ull;
            const int start = (below ? word * 64 + 63 - __clzll((long long)below) : (word > 0 ? sh.last_break[word - 1] : -1)) + 1;
            const int end = above ? word * 64 + __ffsll(above) - 1 : (word < PNG_WORDS - 1 ? sh.next_break[word + 1] : (int)png::PNG_BLOCK_BYTES);
            kind = png::segment_token(i - start, end - start);
        }
        png::Token none = {0u, 0};
        k.token[r] = kind == 0 ? none : (kind == 1 ? png::literal_token(k.byte[r]) : png::match_token(kind));
        upto[r] = k.token[r].len;                       // inclusive prefix sum over the lanes
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int other = __shfl_up(upto[r], s);
            if (lane >= s) upto[r] += other;
        }
        if (lane == 63) sh.word_bits[word] = (uint32_t)upto[r];
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t mine = sh.word_bits[lane];
        uint32_t incl = mine;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t other = __shfl_up(incl, s);
            if (lane >= s) incl += other;
        }
        sh.word_base[lane] = png::BLOCK_HEADER_BITS + incl - mine;
        if (lane == 63) sh.total_bits = png::BLOCK_HEADER_BITS + incl + png::END_OF_BLOCK_BITS;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PNG_ROUNDS; ++r) k.at[r] = sh.word_base[r * (PNG_THREADS / 64) + wave] + (uint32_t)(upto[r] - k.token[r].len);
}

// ORs the low `len` (1..32) bits of `bits` into the stream at bit `pos`, least significant bit first: two words at most
__device__ inline void or_bits_lsb(uint32_t* __restrict__ stream, long long words, unsigned long long pos, uint32_t bits, int len)
{
    const long long w = (long long)(pos >> 5);
    const unsigned long long x = (unsigned long long)(len < 32 ? bits & ((1u << len) - 1) : bits) << (int)(pos & 31);
    const uint32_t w0 = (uint32_t)x, w1 = (uint32_t)(x >> 32);
    if (w0 && w < words) atomicOr(stream + w, w0);
    if (w1 && w + 1 < words) atomicOr(stream + w + 1, w1);
}

__device__ inline void store_byte(uint8_t* __restrict__ files, long long capacity, long long at, uint32_t v)
{
    if (at >= 0 && at < capacity) files[at] = (uint8_t)v;
}

}  // namespace

__global__ __launch_bounds__(PNG_THREADS) void k_png_count(const PngDesc* __restrict__ tab, int batch, int format, int rows, long long total_blocks,
                                                           uint32_t* __restrict__ block_bits, unsigned long long* __restrict__ adler)
{
    __shared__ PngShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (long long g = blockIdx.x; g < total_blocks; g += gridDim.x) {                  // (uniform over the workgroup)
        const int image = last_not_above(batch, g, [&](int i) { return tab[i].block0; });
        const PngDesc& d = tab[image];
        PngWalk k;
        png_walk(d, g - d.block0, format, rows, sh, k);
        unsigned long long s1 = 0, s2 = 0;               // sum R[p] and sum (b1 - p) R[p] over the block: below 2^32
#pragma unroll
        for (int r = 0; r < PNG_ROUNDS; ++r) {
            const int i = r * PNG_THREADS + t;
            if (i < k.len) { s1 += k.byte[r]; s2 += (unsigned long long)(k.len - i) * k.byte[r]; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { s1 += __shfl_xor(s1, s); s2 += __shfl_xor(s2, s); }
        if (lane == 0) { sh.sums[0][wave] = s1; sh.sums[1][wave] = s2; }
        __syncthreads();
        if (t == 0) {
            s1 = 0; s2 = 0;
#pragma unroll
            for (int v = 0; v < PNG_THREADS / 64; ++v) { s1 += sh.sums[0][v]; s2 += sh.sums[1][v]; }
            const long long after = d.n - ((g - d.block0) * png::PNG_BLOCK_BYTES + k.len);
            atomicAdd(adler + 2 * image, (unsigned long long)png::adler_block_a(s1));
            atomicAdd(adler + 2 * image + 1, (unsigned long long)png::adler_block_b(s1, s2, after > 0 ? after : 0));
            block_bits[g] = sh.total_bits;
        }
        __syncthreads();                                 // the next round overwrites sh
    }
}

__global__ __launch_bounds__(1024) void k_png_scan(const PngDesc* __restrict__ tab, int batch, const uint32_t* __restrict__ block_bits,
                                                   long long total_blocks, unsigned long long* __restrict__ block_scan,
                                                   long long* __restrict__ file_offsets)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(block_bits, total_blocks, block_scan, buf);
    const int t = threadIdx.x;
    unsigned long long carry = 0, total;
    for (int base = 0; base < batch; base += 1024) {
        const int i = base + t;
        unsigned long long length = 0;
        if (i < batch) {                                 // an image's stream restarts at bit 0: the difference of two entries of the one scan
            const unsigned long long bits = block_scan[tab[i].block0 + tab[i].blocks] - block_scan[tab[i].block0];
            length = (unsigned long long)tab[i].header_len + png::IDAT_LEAD + ((bits + 7) >> 3) + png::IDAT_TAIL + png::IEND_BYTES;
        }
        const unsigned long long incl = scan_1024(length, buf, &total);
        if (i < batch) file_offsets[i] = (long long)(carry + incl - length);
        carry += total;
    }
    if (t == 0) file_offsets[batch] = (long long)carry;
}

__global__ __launch_bounds__(PNG_THREADS) void k_png_pack(const PngDesc* __restrict__ tab, int batch, int format, int rows, long long total_blocks,
                                                          const unsigned long long* __restrict__ block_scan, const long long* __restrict__ file_offsets,
                                                          uint32_t* __restrict__ files, long long words)
{
    __shared__ PngShared sh;
    for (long long g = blockIdx.x; g < total_blocks; g += gridDim.x) {                  // (uniform over the workgroup)
        const int image = last_not_above(batch, g, [&](int i) { return tab[i].block0; });
        const PngDesc& d = tab[image];
        PngWalk k;
        png_walk(d, g - d.block0, format, rows, sh, k);
        // files start at any byte, so a block's first bit is a position in the whole buffer
        const unsigned long long at = (unsigned long long)(file_offsets[image] + d.header_len + png::IDAT_LEAD) * 8 + (block_scan[g] - block_scan[d.block0]);
        if (threadIdx.x == 0) or_bits_lsb(files, words, at, png::block_header(g == d.block0 + d.blocks - 1), png::BLOCK_HEADER_BITS);
#pragma unroll
        for (int r = 0; r < PNG_ROUNDS; ++r)
            if (k.token[r].len) or_bits_lsb(files, words, at + k.at[r], k.token[r].bits, k.token[r].len);
        __syncthreads();                                 // the next round overwrites sh (the end of block is seven zero bits: already there)
    }
}

__global__ __launch_bounds__(256) void k_png_frame(const PngDesc* __restrict__ tab, int batch, const uint8_t* __restrict__ headers,
                                                   const unsigned long long* __restrict__ adler, const long long* __restrict__ file_offsets,
                                                   uint8_t* __restrict__ files, long long files_capacity)
{
    for (int i = blockIdx.x; i < batch; i += gridDim.x) {
        const long long at = file_offsets[i], end = file_offsets[i + 1];
        const int header_len = tab[i].header_len;
        for (int k = threadIdx.x; k < header_len; k += 256) store_byte(files, files_capacity, at + k, headers[tab[i].header0 + k]);
        const long long data = end - at - header_len - 8 - 4 - png::IEND_BYTES;          // IDAT's data: 78 01, the stream, the Adler-32
        if (threadIdx.x == 0 && data >= 6 && data <= 0x7FFFFFFFll) {
            long long o = at + header_len;
            const uint8_t lead[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
            for (int k = 0; k < 4; ++k) store_byte(files, files_capacity, o++, (uint32_t)(data >> (24 - 8 * k)) & 255u);
            for (int k = 0; k < 6; ++k) store_byte(files, files_capacity, o++, lead[k]);
            const uint32_t sum = png::adler_fold(adler[2 * i], adler[2 * i + 1], tab[i].n);
            o = end - png::IEND_BYTES - 8;
            for (int k = 0; k < 4; ++k) store_byte(files, files_capacity, o++, (sum >> (24 - 8 * k)) & 255u);
            o += 4;                                      // IDAT's CRC-32: the host's, after the copy
            const uint8_t iend[png::IEND_BYTES] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
            for (int k = 0; k < png::IEND_BYTES; ++k) store_byte(files, files_capacity, o++, iend[k]);
        }
    }
}

void png_encode_forward(hipStream_t s, const PngBuffers& b, int batch, long long total_blocks, int format, int rows)
{
    if (batch <= 0 || total_blocks <= 0) return;
    const long long words = b.files_capacity / 4;
    HIP_CHECK(hipMemsetAsync(b.files, 0, (size_t)words * 4, s));
    HIP_CHECK(hipMemsetAsync(b.adler, 0, (size_t)batch * 16, s));
    const int grid = (int)(total_blocks < 65536 ? total_blocks : 65536);
    hipLaunchKernelGGL(k_png_count, dim3(grid), dim3(PNG_THREADS), 0, s, b.tab, batch, format, rows, total_blocks, b.block_bits, b.adler);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(1024), 0, s, b.tab, batch, b.block_bits, total_blocks, b.block_scan, b.file_offsets);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_png_pack, dim3(grid), dim3(PNG_THREADS), 0, s, b.tab, batch, format, rows, total_blocks, b.block_scan, b.file_offsets, b.files, words);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_png_frame, dim3(batch < 1024 ? batch : 1024), dim3(256), 0, s, b.tab, batch, b.headers, b.adler, b.file_offsets,
                       reinterpret_cast<uint8_t*>(b.files), b.files_capacity);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
