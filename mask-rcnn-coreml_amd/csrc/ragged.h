// ragged.h — the host rule of a ragged batch, written once: the sides an image may have and the layout of a ragged output.  Plain C++,
// no HIP header: the host definitions (rle_draw_host.cpp, tiles_host.cpp) and the api*.hip entries check with the same code.  A check
// returns a status and writes its message, which begins with the entry's name, into *err.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/maskrcnn_hip.h"

namespace mrcnn {

inline int bad(std::string* err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int bad(std::string* err, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

// every image's height and width in 1..32767 (MRCNN_ERR_SHAPE naming the image)
inline int check_sides(const int32_t* heights, const int32_t* widths, int n, const char* who, std::string* err)
{
    for (int b = 0; b < n; ++b)
        if (heights[b] < 1 || heights[b] > 32767 || widths[b] < 1 || widths[b] > 32767)
            return bad(err, MRCNN_ERR_SHAPE, "%s: image %d is %dx%d: height and width must lie in 1..32767", who, b, heights[b], widths[b]);
    return MRCNN_OK;
}

// Byte offsets of a ragged output of unit*h_b*w_b bytes per image: each a non-negative multiple of 16, no two ranges overlapping
// (MRCNN_ERR_INVALID).  *extent (may be null) = the largest end.
inline int check_offsets(const int32_t* heights, const int32_t* widths, int n, const int64_t* offsets, int64_t unit, const char* who, int64_t* extent,
                         std::string* err)
{
    if (!offsets) return bad(err, MRCNN_ERR_INVALID, "%s: null output offsets", who);
    auto end_of = [&](int b) { return offsets[b] + unit * heights[b] * widths[b]; };
    int64_t end = 0;
    for (int b = 0; b < n; ++b) {
        if (offsets[b] < 0 || offsets[b] % 16 != 0)
            return bad(err, MRCNN_ERR_INVALID, "%s: image %d: offset %lld is not a non-negative multiple of 16", who, b, (long long)offsets[b]);
        end = end_of(b) > end ? end_of(b) : end;
    }
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (!(end_of(a) <= offsets[b] || end_of(b) <= offsets[a]))
                return bad(err, MRCNN_ERR_INVALID, "%s: images %d and %d overlap in the output", who, a, b);
    if (extent) *extent = end;
    return MRCNN_OK;
}

}  // namespace mrcnn
