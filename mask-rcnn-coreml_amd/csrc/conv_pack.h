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

}  // namespace mrcnn
