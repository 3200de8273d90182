// kernels_jpeg.hip — everything of a JPEG decode behind the entropy decoder, for a ragged batch of files in two launches
// (mrcnn_jpeg_decode_batch, mrcnn_maskrcnn_predict_jpegs):
//   k_jpeg_idct   dequantise + libjpeg's islow 8x8 inverse DCT of every block of every component of every image -> sample planes
//   k_jpeg_color  fancy chroma upsampling + YCbCr -> RGB per output pixel -> interleaved RGB8
// The arithmetic is jpeg_math.h's — the same inline functions the host definition (jpeg_host.cpp) runs — all integer, so the output
// is libjpeg's byte for byte.  Plain HIP C++; built with $(STRICT) like every kernel file that is held to bit equality.
#include "kernels.h"
#include "jpeg_math.h"

namespace mrcnn {

using jpeg::jword;

// the image a batch-wide index falls into: the last entry whose first index (the member at `first`) is <= g
template <long long JpegDesc::*first>
__device__ inline int image_of(const JpegDesc* __restrict__ tab, int batch, long long g)
{
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 256 threads = 32 blocks of 8x8, eight lanes each.  Lane j of a block loads ROW j of the coefficients and of the quantisation table
// (16 bytes each: the wave reads 1 KiB of contiguous coefficients), the products go to LDS; the lane then owns COLUMN j for the first
// pass and row j again for the second, so both passes stay in registers with LDS as the transpose between them and nothing returns
// to memory before the samples.  Rows of 9 words: the row writes and the column reads of a wave fall on 32 distinct banks.
constexpr int IDCT_BLOCKS = 32;
__global__ __launch_bounds__(256) void k_jpeg_idct(const JpegDesc* __restrict__ tab, int batch, const int16_t* __restrict__ coef, long long total_blocks,
                                                   uint8_t* __restrict__ planes)
{
    __shared__ jword ws[IDCT_BLOCKS][8][9];
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    for (long long base = (long long)blockIdx.x * IDCT_BLOCKS; base < total_blocks; base += (long long)gridDim.x * IDCT_BLOCKS) {   // (uniform over the block)
        const long long g = base + slot;
        const bool active = g < total_blocks;
        uint8_t* dst = nullptr;
        jword v[8];
        if (active) {
            const JpegDesc& d = tab[image_of<&JpegDesc::block0>(tab, batch, g)];
            const int c = d.ncomp == 3 ? (g >= d.comp[2].block0 ? 2 : (g >= d.comp[1].block0 ? 1 : 0)) : 0;
            const JpegComp& k = d.comp[c];
            const long long local = g - k.block0;
            const int by = (int)(local / k.blocks_w), bx = (int)(local - (long long)by * k.blocks_w);
            const long long pitch = (long long)k.blocks_w * 8;
            dst = planes + k.plane0 + ((long long)by * 8 + j) * pitch + (long long)bx * 8;
            const uint4 cr = *reinterpret_cast<const uint4*>(coef + g * 64 + j * 8);
            const uint4 qr = *reinterpret_cast<const uint4*>(&d.quant[c][j * 8]);
            const uint32_t cw[4] = {cr.x, cr.y, cr.z, cr.w}, qw[4] = {qr.x, qr.y, qr.z, qr.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ws[slot][j][2 * i] = (jword)(int32_t)(int16_t)(cw[i] & 0xFFFFu) * (jword)(qw[i] & 0xFFFFu);
                ws[slot][j][2 * i + 1] = (jword)(int32_t)(int16_t)(cw[i] >> 16) * (jword)(qw[i] >> 16);
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = ws[slot][r][j];
            jpeg::idct_1d(v, true);
#pragma unroll
            for (int r = 0; r < 8; ++r) ws[slot][r][j] = v[r];       // (the lane's own column: nobody else reads or writes it in this phase)
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = ws[slot][j][i];
            jpeg::idct_1d(v, false);
            uint2 o;
            o.x = (uint32_t)jpeg::idct_sample(v[0]) | (uint32_t)jpeg::idct_sample(v[1]) << 8 | (uint32_t)jpeg::idct_sample(v[2]) << 16 |
                  (uint32_t)jpeg::idct_sample(v[3]) << 24;
            o.y = (uint32_t)jpeg::idct_sample(v[4]) | (uint32_t)jpeg::idct_sample(v[5]) << 8 | (uint32_t)jpeg::idct_sample(v[6]) << 16 |
                  (uint32_t)jpeg::idct_sample(v[7]) << 24;
            *reinterpret_cast<uint2*>(dst) = o;      // (plane0 is a multiple of 16 and the pitch of 8: aligned)
        }
        __syncthreads();                             // the next round overwrites ws
    }
}

// One thread = 16 consecutive pixels of an image's flat h*w order = 48 bytes of its RGB8 output, which start on a 16-byte boundary
// whenever the image does: three 16-byte stores.  The last, partial chunk of an image — and every chunk of an image whose output is
// not 16-byte aligned — goes out byte by byte, so no byte outside the image's h*w*3 is ever written.
__global__ __launch_bounds__(256) void k_jpeg_color(const JpegDesc* __restrict__ tab, int batch, const uint8_t* __restrict__ planes, long long total_chunks,
                                                    uint8_t* __restrict__ out)
{
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total_chunks; g += (long long)gridDim.x * 256) {
        const JpegDesc& d = tab[image_of<&JpegDesc::chunk0>(tab, batch, g)];
        const long long p0 = (g - d.chunk0) * 16, npix = (long long)d.h * d.w;
        const int n = npix - p0 < 16 ? (int)(npix - p0) : 16;
        jpeg::Planes p;
        p.ncomp = d.ncomp; p.mode = d.mode;
        p.cw = d.comp[d.ncomp - 1].width; p.ch = d.comp[d.ncomp - 1].height;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const JpegComp& k = d.comp[c < d.ncomp ? c : 0];
            p.plane[c] = planes + k.plane0;
            p.pitch[c] = (long long)k.blocks_w * 8;
        }
        int y = (int)(p0 / d.w), x = (int)(p0 - (long long)y * d.w);
        uint32_t words[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < n) {
                const uint32_t v = jpeg::pixel_rgb(p, x, y);         // R | G << 8 | B << 16, at byte 3k of the 48
                words[(3 * k) >> 2] |= v << (8 * ((3 * k) & 3));
                if ((3 * k) & 3) words[((3 * k) >> 2) + 1] |= v >> (32 - 8 * ((3 * k) & 3));     // (k = 15 ends on the last word: its spill is zero bits, never indexed)
                if (++x == d.w) { x = 0; ++y; }
            }
        }
        uint8_t* dst = out + d.out_offset + p0 * 3;
        if (n == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            uint4* q = reinterpret_cast<uint4*>(dst);
            q[0] = make_uint4(words[0], words[1], words[2], words[3]);
            q[1] = make_uint4(words[4], words[5], words[6], words[7]);
            q[2] = make_uint4(words[8], words[9], words[10], words[11]);
        } else {
#pragma unroll
            for (int i = 0; i < 48; ++i)
                if (i < 3 * n) dst[i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
        }
    }
}

static int capped_grid(long long work_groups)
{
    return (int)(work_groups < 1 ? 1 : (work_groups < 4096 ? work_groups : 4096));
}

void jpeg_decode_forward(hipStream_t s, const JpegDesc* tab, int batch, const int16_t* coef, long long total_blocks, uint8_t* planes,
                         long long total_chunks, uint8_t* out)
{
    if (batch <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(k_jpeg_idct, dim3(capped_grid((total_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(256), 0, s, tab, batch, coef, total_blocks, planes);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jpeg_color, dim3(capped_grid((total_chunks + 255) / 256)), dim3(256), 0, s, tab, batch, planes, total_chunks, out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
