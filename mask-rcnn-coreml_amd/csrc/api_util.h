// api_util.h — what more than one api*.hip translation unit needs: row staging between the caller's memory space and
// dense device buffers, an owned stream and the guard that drains one, rounding up, one scratch carver, and the staging of a ragged batch
// (ragged.h is its host rule): the image table's sizes, the sources' upload and the output.  Header-only; internal linkage, nothing here is exported.
#pragma once
#include <vector>

#include "engine.h"
#include "ragged.h"

namespace mrcnn {

// Copies n rows of `len` floats (source row stride `stride` elements) into a dense device buffer.
static const float* stage_rows(const void* src, int memspace, long n, long len, long stride, DevBuf& tmp)
{
    if (memspace == MRCNN_DEVICE && stride == len) return static_cast<const float*>(src);
    tmp.alloc((size_t)(n > 0 ? n : 1) * len * 4);
    if (n <= 0) return tmp.as<float>();
    HIP_CHECK(hipMemcpy2D(tmp.p, (size_t)len * 4, src, (size_t)stride * 4, (size_t)len * 4, (size_t)n,
                          memspace == MRCNN_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return tmp.as<float>();
}

// Writes n dense device rows of `len` floats to a destination with row stride `stride`.
static void unstage_rows(const float* dev, void* dst, int memspace, long n, long len, long stride)
{
    if (n <= 0) return;
    HIP_CHECK(hipMemcpy2D(dst, (size_t)stride * 4, dev, (size_t)len * 4, (size_t)len * 4, (size_t)n,
                          memspace == MRCNN_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
}

struct Stream {
    hipStream_t s = nullptr;
    Stream() { require_gpu(); HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

// Synchronises `s` when the scope ends, however it ends: an error after work was queued must not leave it running on staging or scratch
// that the next call rewrites.
struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
};

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the answer of a host check (ragged.h, rle_draw_host.h, tiles_host.h) as this library's error
static void answer(int st, const std::string& err)
{
    if (st != MRCNN_OK) fail(st, "%s", err.c_str());
}

// the sizes of the images of a table, null pointers refused
static void image_sizes(const mrcnn_image* images, int n_images, const char* who, std::vector<int32_t>& hs, std::vector<int32_t>& ws)
{
    MRCNN_REQUIRE(images, MRCNN_ERR_INVALID, "%s: null images", who);
    MRCNN_REQUIRE(n_images >= 0, MRCNN_ERR_INVALID, "%s: n_images %d is negative", who, n_images);
    hs.assign((size_t)n_images, 0); ws.assign((size_t)n_images, 0);
    for (int b = 0; b < n_images; ++b) {
        MRCNN_REQUIRE(images[b].rgb, MRCNN_ERR_INVALID, "%s: image %d has a null rgb pointer", who, b);
        hs[(size_t)b] = images[b].height; ws[(size_t)b] = images[b].width;
    }
}

// One device allocation carved into typed arrays, each from a 16-byte boundary: take<T>(n) for every array, alloc(), then carve[slot].
struct Carver {
    template <class T> struct Slot { size_t at; };
    size_t size = 0;
    DevBuf buf;
    template <class T> Slot<T> take(size_t n) { const Slot<T> s{size}; size = up(size + n * sizeof(T), 16); return s; }
    void alloc() { buf.alloc(size); }
    template <class T> T* operator[](Slot<T> s) const { return reinterpret_cast<T*>(buf.as<char>() + s.at); }
};

// image b's own unit*h_b*w_b bytes of a ragged output, from a device copy at the caller's offsets (ragged.h) to the host caller
static void ragged_to_host(void* callers, const uint8_t* staged, const int64_t* offsets, const int32_t* hs, const int32_t* ws, int n, int64_t unit)
{
    for (int b = 0; b < n; ++b)
        HIP_CHECK(hipMemcpy(static_cast<uint8_t*>(callers) + offsets[b], staged + offsets[b], (size_t)(unit * hs[b] * ws[b]), hipMemcpyDeviceToHost));
}

// A ragged output of work queued on `s`: p, where the kernels write, is the caller's device buffer or a staging copy with the same
// offsets.  Declare it behind the call's other buffers: the stream drains before any of them is freed.
struct RaggedOut {
    uint8_t* p;
    DevBuf tmp;
    Drain drain;
    RaggedOut(hipStream_t s, void* callers, bool dev, int64_t extent) : p(static_cast<uint8_t*>(callers)), drain{s}
    {
        if (!dev) { tmp.alloc((size_t)extent); p = tmp.as<uint8_t>(); }
    }
    // the stream is synchronised: only the images' own bytes go to a host caller
    void deliver(void* callers, const int64_t* offsets, const int32_t* hs, const int32_t* ws, int n, int64_t unit) const
    {
        if (tmp.p) ragged_to_host(callers, p, offsets, hs, ws, n, unit);
    }
};

// The sources of a render entry as a device array of pointers at `table`: the caller's own for MRCNN_DEVICE, otherwise uploaded into
// `pixels` back to back, each from a 16-byte boundary.
static void upload_sources(const mrcnn_image* images, int n, bool dev, DevBuf& pixels, const uint8_t** table)
{
    std::vector<const uint8_t*> srcs((size_t)n);
    auto bytes_of = [&](int b) { return (size_t)3 * images[b].height * images[b].width; };
    size_t total = 0, at = 0;
    for (int b = 0; b < n; ++b) total += up(bytes_of(b), 16);
    if (!dev) pixels.alloc(total);
    for (int b = 0; b < n; ++b) {
        srcs[(size_t)b] = images[b].rgb;
        if (dev) continue;
        HIP_CHECK(hipMemcpy(pixels.as<uint8_t>() + at, images[b].rgb, bytes_of(b), hipMemcpyHostToDevice));
        srcs[(size_t)b] = pixels.as<uint8_t>() + at;
        at += up(bytes_of(b), 16);
    }
    HIP_CHECK(hipMemcpy(table, srcs.data(), srcs.size() * sizeof(const uint8_t*), hipMemcpyHostToDevice));
}

}  // namespace mrcnn
