// kernels_jpeg_enc.hip — a baseline JPEG encoder for a ragged batch of RGB8 images, every stage on the device
// (mrcnn_jpeg_encode_batch); the number of launches does not depend on the batch:
//   k_jpeg_fdct         RGB -> YCbCr, chroma downsampling, jfdctint, quantisation -> int16 coefficients, zigzag, scan order
//   k_jpeg_count        one wave per block: the bits its Huffman codes take
//   k_jpeg_scan_blocks  exclusive scan of those (one block) + where each image's scan starts in the word stream
//   k_jpeg_pack         the same walk: every lane ORs its code into the zeroed stream
//   k_jpeg_ffcount      FF bytes per chunk of the stream
//   k_jpeg_scan_chunks  their scan (one block) + the offsets of the finished files
//   k_jpeg_stuff        the scan's bytes behind each file's header, a zero after every FF
//   k_jpeg_frame        the headers (built on the host) and the EOI markers
// The arithmetic and the code words are jpeg_math.h's — the inline functions the host definition (jpeg_enc_host.cpp) runs — so the
// files equal mrcnn_jpeg_encode_host's byte for byte.  Plain HIP C++, vector stores and vector atomics only; every loop is bounded by
// a kernel argument (a size read from device memory is clamped to one).
#include "kernels.h"
#include "jpeg_math.h"
#include "scan_device.h"

namespace mrcnn {

namespace {

struct EncBlock {
    int image, c, bx, by;      // component, and the block's place on the component's grid
    long long prev;            // the block before it of the same component in scan order (its DC predictor), -1 = none
};
__device__ inline EncBlock enc_block(const JpegEncDesc* __restrict__ tab, int batch, long long g)
{
    EncBlock e;
    e.image = last_not_above(batch, g, [&](int i) { return tab[i].block0; });
    const JpegEncDesc& d = tab[e.image];
    const long long local = g - d.block0, mcu = local / d.blocks_per_mcu;
    const int k = (int)(local - mcu * d.blocks_per_mcu), luma = d.ncomp == 1 ? 1 : d.hs * d.vs;
    const int my = (int)(mcu / d.mcus_x), mx = (int)(mcu - (long long)my * d.mcus_x);
    if (k < luma) {
        e.c = 0;
        e.bx = mx * d.hs + k % d.hs;
        e.by = my * d.vs + k / d.hs;
        e.prev = k > 0 ? g - 1 : (mcu > 0 ? g - d.blocks_per_mcu + luma - 1 : -1);
    } else {
        e.c = k - luma + 1;
        e.bx = mx;
        e.by = my;
        e.prev = mcu > 0 ? g - d.blocks_per_mcu : -1;
    }
    return e;
}

// what lane `lane` (= zigzag position) of a block's wave appends to the scan: lane 0 the DC difference, a lane with a non-zero
// coefficient its ZRLs, code and bits — the zero run read off the ballot of non-zero lanes —, lane 63 the EOB when its coefficient is zero
__device__ inline jpeg::Code lane_code(const JpegEncHuffman* __restrict__ huff, int table, int lane, int v, int pred, unsigned long long nonzero_ac)
{
    if (lane == 0) return jpeg::code_dc(huff->dc[table], v - pred);
    if (v != 0) {
        const unsigned long long below = nonzero_ac & ((1ull << lane) - 1);
        const int before = below ? 63 - __clzll((long long)below) : 0;
        return jpeg::code_ac(huff->ac[table], lane - before - 1, v);
    }
    if (lane == 63) return jpeg::code_eob(huff->ac[table]);
    jpeg::Code none = {0, 0};
    return none;
}

// ORs the low `len` (1..64) bits of `bits` into the stream at bit `pos`, most significant bit first: three words at most
__device__ inline void or_bits(uint32_t* __restrict__ stream, long long words, unsigned long long pos, unsigned long long bits, int len)
{
    const unsigned long long x = bits << (64 - len);                // left-aligned
    const long long w = (long long)(pos >> 5);
    const int s = (int)(pos & 31);
    const unsigned long long rest = s ? x << (32 - s) : 0;          // what the first word did not take: 32 + s bits, left-aligned
    const uint32_t w0 = (uint32_t)(x >> (32 + s));
    const uint32_t w1 = s ? (uint32_t)(rest >> 32) : (uint32_t)x;
    const uint32_t w2 = s ? (uint32_t)rest : 0u;
    if (w0 && w < words) atomicOr(stream + w, w0);
    if (w1 && w + 1 < words) atomicOr(stream + w + 1, w1);
    if (w2 && w + 2 < words) atomicOr(stream + w + 2, w2);
}

__device__ inline uint32_t stream_byte(const uint32_t* __restrict__ stream, long long k)
{
    return (stream[k >> 2] >> (24 - 8 * (int)(k & 3))) & 255u;
}

}  // namespace

// 256 threads = 32 blocks of 8x8, eight lanes each (k_jpeg_idct's mapping, run backwards).  Lane j gathers ROW j of its block's
// samples — RGB read with the edge clamped, converted and box-filtered on the way, so the converted planes never exist in memory —
// and runs the row pass in registers; LDS (rows of 9 words: a wave's row writes and column reads fall on distinct banks) transposes;
// the lane runs the pass over COLUMN j and quantises; LDS again puts the 64 values into zigzag order and the lane stores 16 bytes.
constexpr int FDCT_BLOCKS = 32;
__global__ __launch_bounds__(256) void k_jpeg_fdct(const JpegEncDesc* __restrict__ tab, int batch, const JpegEncHuffman* __restrict__ huff,
                                                   long long total_blocks, int16_t* __restrict__ coef)
{
    __shared__ int32_t ws[FDCT_BLOCKS][8][9];
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    for (long long base = (long long)blockIdx.x * FDCT_BLOCKS; base < total_blocks; base += (long long)gridDim.x * FDCT_BLOCKS) {   // (uniform over the block)
        const long long g = base + slot;
        const bool active = g < total_blocks;
        int32_t v[8];
        const uint16_t* quant = nullptr;
        if (active) {
            const EncBlock e = enc_block(tab, batch, g);
            const JpegEncDesc& d = tab[e.image];
            quant = d.quant[e.c ? 1 : 0];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = jpeg::enc_sample(d.rgb, d.h, d.w, d.sampling, e.c, e.bx * 8 + i, e.by * 8 + j) - 128;
            jpeg::fdct_1d(v, true);
#pragma unroll
            for (int i = 0; i < 8; ++i) ws[slot][j][i] = v[i];
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = ws[slot][r][j];
            jpeg::fdct_1d(v, false);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = jpeg::quantise(v[r], quant[r * 8 + j]);
        }
        __syncthreads();                                 // every column is read before the zigzag order overwrites the block
        if (active) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int z = huff->zigzag_of[r * 8 + j];
                ws[slot][z >> 3][z & 7] = v[r];
            }
        }
        __syncthreads();
        if (active) {
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = ((uint32_t)ws[slot][j][2 * i] & 0xFFFFu) | (uint32_t)ws[slot][j][2 * i + 1] << 16;
            *reinterpret_cast<uint4*>(coef + g * 64 + j * 8) = make_uint4(o[0], o[1], o[2], o[3]);     // (coef is 16-byte aligned)
        }
        __syncthreads();                                 // the next round overwrites ws
    }
}

// One wave64 per block, lane k = zigzag coefficient k; four blocks per thread block.
__global__ __launch_bounds__(256) void k_jpeg_count(const JpegEncDesc* __restrict__ tab, int batch, const JpegEncHuffman* __restrict__ huff,
                                                    const int16_t* __restrict__ coef, long long total_blocks, uint32_t* __restrict__ block_bits)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long g = (long long)blockIdx.x * 4 + wave; g < total_blocks; g += (long long)gridDim.x * 4) {      // (uniform over the wave)
        const EncBlock e = enc_block(tab, batch, g);
        const int v = coef[g * 64 + lane];
        const int pred = lane == 0 && e.prev >= 0 ? coef[e.prev * 64] : 0;
        const unsigned long long nonzero_ac = __ballot(v != 0) & ~1ull;
        int bits = lane_code(huff, e.c ? 1 : 0, lane, v, pred, nonzero_ac).len;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) bits += __shfl_xor(bits, d);
        if (lane == 0) block_bits[g] = (uint32_t)bits;
    }
}

__global__ __launch_bounds__(1024) void k_jpeg_scan_blocks(const JpegEncDesc* __restrict__ tab, int batch, const uint32_t* __restrict__ block_bits,
                                                           long long total_blocks, unsigned long long* __restrict__ block_scan,
                                                           long long* __restrict__ image_chunk0, long long* __restrict__ image_bytes)
{
    __shared__ unsigned long long buf[2][1024];
    scan_array(block_bits, total_blocks, block_scan, buf);
    const int t = threadIdx.x;
    unsigned long long carry = 0, total;
    for (int base = 0; base < batch; base += 1024) {
        const int i = base + t;
        unsigned long long chunks = 0;
        if (i < batch) {
            const unsigned long long bits = block_scan[tab[i].block0 + tab[i].blocks] - block_scan[tab[i].block0];
            const unsigned long long bytes = (bits + 7) >> 3;
            image_bytes[i] = (long long)bytes;
            chunks = (bytes + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
        }
        const unsigned long long incl = scan_1024(chunks, buf, &total);
        if (i < batch) image_chunk0[i] = (long long)(carry + incl - chunks);
        carry += total;
    }
    if (t == 0) image_chunk0[batch] = (long long)carry;
}

__global__ __launch_bounds__(256) void k_jpeg_pack(const JpegEncDesc* __restrict__ tab, int batch, const JpegEncHuffman* __restrict__ huff,
                                                   const int16_t* __restrict__ coef, long long total_blocks,
                                                   const unsigned long long* __restrict__ block_scan, const long long* __restrict__ image_chunk0,
                                                   uint32_t* __restrict__ stream, long long words)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long g = (long long)blockIdx.x * 4 + wave; g < total_blocks; g += (long long)gridDim.x * 4) {      // (uniform over the wave)
        const EncBlock e = enc_block(tab, batch, g);
        const JpegEncDesc& d = tab[e.image];
        const int v = coef[g * 64 + lane];
        const int pred = lane == 0 && e.prev >= 0 ? coef[e.prev * 64] : 0;
        const unsigned long long nonzero_ac = __ballot(v != 0) & ~1ull;
        const jpeg::Code c = lane_code(huff, e.c ? 1 : 0, lane, v, pred, nonzero_ac);
        int upto = c.len;                                // inclusive prefix sum over the lanes
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int other = __shfl_up(upto, s);
            if (lane >= s) upto += other;
        }
        const unsigned long long image_bit0 = (unsigned long long)image_chunk0[e.image] * (JPEG_ENC_CHUNK * 8);
        const unsigned long long at = image_bit0 + (block_scan[g] - block_scan[d.block0]);
        if (c.len) or_bits(stream, words, at + (unsigned long long)(upto - c.len), c.bits, c.len);
        if (lane == 63 && g == d.block0 + d.blocks - 1) {          // the image's last byte is filled with 1-bits
            const unsigned long long end = at + (unsigned long long)upto;
            const int pad = (int)((8 - (end & 7)) & 7);
            if (pad) or_bits(stream, words, end, (1ull << pad) - 1, pad);
        }
    }
}

// chunk -> its image and the bytes of it that are scan data
struct EncChunk { int image; int bytes; long long local; };
__device__ inline EncChunk enc_chunk(const long long* __restrict__ image_chunk0, const long long* __restrict__ image_bytes, int batch, long long ch)
{
    EncChunk k;
    k.image = last_not_above(batch, ch, [&](int i) { return image_chunk0[i]; });
    k.local = ch - image_chunk0[k.image];
    const long long left = image_bytes[k.image] - k.local * JPEG_ENC_CHUNK;
    k.bytes = (int)(left < JPEG_ENC_CHUNK ? (left > 0 ? left : 0) : JPEG_ENC_CHUNK);
    return k;
}
__device__ inline long long used_chunks(const long long* __restrict__ image_chunk0, int batch, long long max_chunks)
{
    const long long n = image_chunk0[batch];
    return n < max_chunks ? n : max_chunks;
}

__global__ __launch_bounds__(256) void k_jpeg_ffcount(const uint32_t* __restrict__ stream, const long long* __restrict__ image_chunk0,
                                                      const long long* __restrict__ image_bytes, int batch, long long max_chunks,
                                                      uint32_t* __restrict__ chunk_ff)
{
    const long long n = used_chunks(image_chunk0, batch, max_chunks);
    for (long long ch = (long long)blockIdx.x * 256 + threadIdx.x; ch < n; ch += (long long)gridDim.x * 256) {
        const EncChunk k = enc_chunk(image_chunk0, image_bytes, batch, ch);
        uint32_t count = 0;
        for (int i = 0; i < JPEG_ENC_CHUNK; ++i)
            if (i < k.bytes && stream_byte(stream, ch * JPEG_ENC_CHUNK + i) == 255u) ++count;
        chunk_ff[ch] = count;
    }
}

__global__ __launch_bounds__(1024) void k_jpeg_scan_chunks(const JpegEncDesc* __restrict__ tab, int batch, const uint32_t* __restrict__ chunk_ff,
                                                           long long max_chunks, const long long* __restrict__ image_chunk0,
                                                           const long long* __restrict__ image_bytes, unsigned long long* __restrict__ chunk_scan,
                                                           long long* __restrict__ file_offsets)
{
    __shared__ unsigned long long buf[2][1024];
    const long long n = used_chunks(image_chunk0, batch, max_chunks);
    scan_array(chunk_ff, n, chunk_scan, buf);
    const int t = threadIdx.x;
    unsigned long long carry = 0, total;
    for (int base = 0; base < batch; base += 1024) {
        const int i = base + t;
        unsigned long long length = 0;
        if (i < batch) {
            const long long c0 = image_chunk0[i] < n ? image_chunk0[i] : n, c1 = image_chunk0[i + 1] < n ? image_chunk0[i + 1] : n;
            length = (unsigned long long)tab[i].header_len + (unsigned long long)image_bytes[i] + (chunk_scan[c1] - chunk_scan[c0]) + 2;
        }
        const unsigned long long incl = scan_1024(length, buf, &total);
        if (i < batch) file_offsets[i] = (long long)(carry + incl - length);
        carry += total;
    }
    if (t == 0) file_offsets[batch] = (long long)carry;
}

__global__ __launch_bounds__(256) void k_jpeg_stuff(const JpegEncDesc* __restrict__ tab, int batch, const uint32_t* __restrict__ stream,
                                                    const long long* __restrict__ image_chunk0, const long long* __restrict__ image_bytes,
                                                    long long max_chunks, const unsigned long long* __restrict__ chunk_scan,
                                                    const long long* __restrict__ file_offsets, uint8_t* __restrict__ files, long long files_capacity)
{
    const long long n = used_chunks(image_chunk0, batch, max_chunks);
    for (long long ch = (long long)blockIdx.x * 256 + threadIdx.x; ch < n; ch += (long long)gridDim.x * 256) {
        const EncChunk k = enc_chunk(image_chunk0, image_bytes, batch, ch);
        long long o = file_offsets[k.image] + tab[k.image].header_len + k.local * JPEG_ENC_CHUNK +
                      (long long)(chunk_scan[ch] - chunk_scan[image_chunk0[k.image]]);
        for (int i = 0; i < JPEG_ENC_CHUNK; ++i) {
            if (i >= k.bytes) break;
            const uint32_t b = stream_byte(stream, ch * JPEG_ENC_CHUNK + i);
            if (o < files_capacity) files[o] = (uint8_t)b;
            ++o;
            if (b == 255u) {
                if (o < files_capacity) files[o] = 0;
                ++o;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_frame(const JpegEncDesc* __restrict__ tab, int batch, const uint8_t* __restrict__ headers,
                                                    const long long* __restrict__ file_offsets, uint8_t* __restrict__ files, long long files_capacity)
{
    for (int i = blockIdx.x; i < batch; i += gridDim.x) {
        const long long at = file_offsets[i], end = file_offsets[i + 1];
        for (int k = threadIdx.x; k < tab[i].header_len; k += 256)
            if (at + k < files_capacity) files[at + k] = headers[tab[i].header0 + k];
        if (threadIdx.x == 0 && end >= 2 && end <= files_capacity) {
            files[end - 2] = 0xFF;
            files[end - 1] = 0xD9;
        }
    }
}

static int capped_grid(long long work_groups)
{
    return (int)(work_groups < 1 ? 1 : (work_groups < 4096 ? work_groups : 4096));
}

void jpeg_encode_forward(hipStream_t s, const JpegEncBuffers& b, int batch, long long total_blocks)
{
    if (batch <= 0 || total_blocks <= 0) return;
    const long long words = b.max_chunks * (JPEG_ENC_CHUNK / 4);
    HIP_CHECK(hipMemsetAsync(b.stream, 0, (size_t)words * 4, s));
    hipLaunchKernelGGL(k_jpeg_fdct, dim3(capped_grid((total_blocks + FDCT_BLOCKS - 1) / FDCT_BLOCKS)), dim3(256), 0, s, b.tab, batch, b.huff, total_blocks, b.coef);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_count, dim3(capped_grid((total_blocks + 3) / 4)), dim3(256), 0, s, b.tab, batch, b.huff, b.coef, total_blocks, b.block_bits);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_scan_blocks, dim3(1), dim3(1024), 0, s, b.tab, batch, b.block_bits, total_blocks, b.block_scan, b.image_chunk0, b.image_bytes);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_pack, dim3(capped_grid((total_blocks + 3) / 4)), dim3(256), 0, s, b.tab, batch, b.huff, b.coef, total_blocks, b.block_scan,
                       b.image_chunk0, b.stream, words);
    HIP_CHECK(hipGetLastError());
    const int chunk_grid = capped_grid((b.max_chunks + 255) / 256);
    hipLaunchKernelGGL(k_jpeg_ffcount, dim3(chunk_grid), dim3(256), 0, s, b.stream, b.image_chunk0, b.image_bytes, batch, b.max_chunks, b.chunk_ff);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_scan_chunks, dim3(1), dim3(1024), 0, s, b.tab, batch, b.chunk_ff, b.max_chunks, b.image_chunk0, b.image_bytes, b.chunk_scan,
                       b.file_offsets);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_stuff, dim3(chunk_grid), dim3(256), 0, s, b.tab, batch, b.stream, b.image_chunk0, b.image_bytes, b.max_chunks, b.chunk_scan,
                       b.file_offsets, b.files, b.files_capacity);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_frame, dim3(batch < 1024 ? batch : 1024), dim3(256), 0, s, b.tab, batch, b.headers, b.file_offsets, b.files, b.files_capacity);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
