// api_util.h — what more than one api*.hip translation unit needs: row staging between the caller's memory space and
// dense device buffers, an owned stream and the guard that drains one, and rounding up.  Header-only; internal linkage, nothing here is exported.
#pragma once
#include "engine.h"

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

}  // namespace mrcnn
