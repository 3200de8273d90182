// conv_pack.h — the ONE statement of the filter layouts conv_forward reads (ConvDesc::wgt), as host routines over any source
// layout: the engine's packers (engine_weights.hip: Core ML's [O][I][KH][KW] / [I][O][2][2]) and the test entry on caller data
// (api_test.hip: mrcnn_test_conv_form_nhwc) both call these, each with the accessor of its own source.  Header-only, no HIP.
#pragma once
#include <stddef.h>
#include <vector>

namespace mrcnn {

// [Npad][KH][KW][I], k contiguous (tap-major, channel-minor), rows O..Npad-1 zero; src(o, y, x, i) = the filter value
template <class Src>
std::vector<float> pack_filter_rows(int O, int I, int KH, int KW, int Npad, Src&& src)
{
    std::vector<float> w((size_t)Npad * KH * KW * I, 0.f);
    for (int o = 0; o < O; ++o)
        for (int y = 0; y < KH; ++y)
            for (int x = 0; x < KW; ++x)
                for (int i = 0; i < I; ++i) w[(((size_t)o * KH + y) * KW + x) * I + i] = src(o, y, x, i);
    return w;
}

// ConvTranspose 2x2 stride 2 as a GEMM: row n = (dy*2 + dx)*O + co feeds output pixel (2oh + dy, 2ow + dx), channel co
inline int deconv2_row(int dy, int dx, int co, int O) { return (dy * 2 + dx) * O + co; }
// [Npad][I] with Npad >= 4*O, rows beyond 4*O zero; src(dy, dx, co, i) = the kernel value
template <class Src>
std::vector<float> pack_deconv2_rows(int I, int O, int Npad, Src&& src)
{
    std::vector<float> w((size_t)Npad * I, 0.f);
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx)
            for (int o = 0; o < O; ++o)
                for (int i = 0; i < I; ++i) w[(size_t)deconv2_row(dy, dx, o, O) * I + i] = src(dy, dx, o, i);
    return w;
}

// Stream images of a chainable pointwise pair at C = 256 (kernels_conv_chain.hip, the ring form): P = branch2c, [4C][C], Q = the next
// block's branch2a, [C][4C].  The kernel walks P's columns in chunks of 64, and a chunk of P's columns is a chunk of Q's channels: per chunk
// it copies 64 rows x C channels of P's filter and C rows x 64 channels of Q's into LDS by DMA, a straight copy — so a chunk's image lies
// contiguous in memory in exactly its LDS layout, the 128-row kernel's: [K step of 32 channels][row][64 B], the 16-B piece c of row r at
// piece position c ^ ((r >> 2) & 3).  An image is [4C / 64 chunks][64 * C elements]; the position of filter element (row n, channel k):
inline bool chain_stream_wanted(int KH, int KW, int I, int O) { return KH == 1 && KW == 1 && ((I == 256 && O == 1024) || (I == 1024 && O == 256)); }
inline size_t chain_stream_pos_p(int C, int n, int k)
{
    const int r = n & 63;
    return (size_t)(n >> 6) * 64 * C + ((size_t)(k >> 5) * 64 + r) * 32 + ((((k >> 3) & 3) ^ ((r >> 2) & 3)) << 3) + (k & 7);
}
inline size_t chain_stream_pos_q(int C, int n, int k)
{
    return (size_t)(k >> 6) * 64 * C + ((size_t)((k >> 5) & 1) * C + n) * 32 + ((((k >> 3) & 3) ^ ((n >> 2) & 3)) << 3) + (k & 7);
}
// w: the layer's filter rows as conv_forward reads them ([4C][C] for P, q = false; [C][4C] for Q, q = true), any 2-byte element type
template <class T>
std::vector<T> pack_chain_stream(const T* w, int C, bool q)
{
    static_assert(sizeof(T) == 2, "fp16 filters");
    const int rows = q ? C : 4 * C, K = q ? 4 * C : C;
    std::vector<T> img((size_t)rows * K);
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < K; ++k) img[q ? chain_stream_pos_q(C, n, k) : chain_stream_pos_p(C, n, k)] = w[(size_t)n * K + k];
    return img;
}

}  // namespace mrcnn
