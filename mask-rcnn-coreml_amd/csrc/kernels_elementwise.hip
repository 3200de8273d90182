// kernels_elementwise.hip — the small element-wise kernels around the convolution family: preprocessing, the stem's max-pool,
// the soft-maxes, layout changes, and the mask head's row selection (declared with the family in kernels.h).
#include "conv_device.h"

namespace mrcnn {

// ================================================================================================
// element-wise helpers
// ================================================================================================
// fp32: NHWC4 (16 B per pixel); fp16: NHWC8 (16 B per pixel) — either way one 16-B store per pixel
template <typename T>
__global__ __launch_bounds__(256) void k_preprocess(const uint8_t* __restrict__ rgb, int B, int H, int W, int pad,
                                                    float mr, float mg, float mb, void* __restrict__ out)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const long total = (long)B * Hp * Wp;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int x = (int)(e % Wp);
        const int y = (int)((e / Wp) % Hp);
        const int b = (int)(e / ((long)Wp * Hp));
        float r = 0.f, g = 0.f, bl = 0.f;
        const int sy = y - pad, sx = x - pad;
        if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) {
            const uint8_t* p = rgb + (((long)b * H + sy) * W + sx) * 3;
            r = (float)p[0] - mr; g = (float)p[1] - mg; bl = (float)p[2] - mb;
        }
        if constexpr (sizeof(T) == 4) {
            reinterpret_cast<float4*>(out)[e] = make_float4(r, g, bl, 0.f);
        } else {
            f16x8 h;
            h[0] = (_Float16)r; h[1] = (_Float16)g; h[2] = (_Float16)bl;
            h[3] = h[4] = h[5] = h[6] = h[7] = (_Float16)0.f;
            reinterpret_cast<f16x8*>(out)[e] = h;
        }
    }
}

void preprocess_forward(hipStream_t s, const uint8_t* rgb, int B, int H, int W, int pad, const float mean[3], void* out, int dtype)
{
    const long total = (long)B * (H + 2 * pad) * (W + 2 * pad);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (dtype == MRCNN_F16) hipLaunchKernelGGL(k_preprocess<_Float16>, dim3(grid), dim3(256), 0, s, rgb, B, H, W, pad, mean[0], mean[1], mean[2], out);
    else hipLaunchKernelGGL(k_preprocess<float>, dim3(grid), dim3(256), 0, s, rgb, B, H, W, pad, mean[0], mean[1], mean[2], out);
    HIP_CHECK(hipGetLastError());
}

template <typename T>
__global__ __launch_bounds__(256) void k_maxpool3x3s2(const T* __restrict__ in, int B, int H, int W, int C4,
                                                      T* __restrict__ out, int OH, int OW)
{
    const long total = (long)B * OH * OW * C4;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C4);
        const int ox = (int)((e / C4) % OW);
        const int oy = (int)((e / ((long)C4 * OW)) % OH);
        const int b = (int)(e / ((long)C4 * OW * OH));
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dy = 0; dy < 3; ++dy) {
            const int y = 2 * oy + dy;
            if (y >= H) break;
            for (int dx = 0; dx < 3; ++dx) {
                const int x = 2 * ox + dx;
                if (x >= W) break;
                const float4 v = load4<T>(in + ((((long)b * H + y) * W + x) * C4 + c) * 4);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        store4<T>(out + e * 4, m);
    }
}

void maxpool3x3s2_forward(hipStream_t s, const void* in, int B, int H, int W, int C, void* out, int OH, int OW, int dtype)
{
    MRCNN_REQUIRE(C % 4 == 0, MRCNN_ERR_SHAPE, "maxpool: C %% 4 != 0");
    const long total = (long)B * OH * OW * (C / 4);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (dtype == MRCNN_F16)
        hipLaunchKernelGGL(k_maxpool3x3s2<_Float16>, dim3(grid), dim3(256), 0, s, (const _Float16*)in, B, H, W, C / 4, (_Float16*)out, OH, OW);
    else hipLaunchKernelGGL(k_maxpool3x3s2<float>, dim3(grid), dim3(256), 0, s, (const float*)in, B, H, W, C / 4, (float*)out, OH, OW);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_softmax_pairs(const float2* __restrict__ logits, float2* __restrict__ probs, long n)
{
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float2 l = logits[e];
        const float m = fmaxf(l.x, l.y);
        const float e0 = expf(l.x - m), e1 = expf(l.y - m);
        const float inv = 1.0f / (e0 + e1);
        probs[e] = make_float2(e0 * inv, e1 * inv);
    }
}

void softmax_pairs_forward(hipStream_t s, const float* logits, float* probs, long n_pairs)
{
    const int grid = (int)((n_pairs + 255) / 256 < 8192 ? (n_pairs + 255) / 256 : 8192);
    hipLaunchKernelGGL(k_softmax_pairs, dim3(grid), dim3(256), 0, s, (const float2*)logits, (float2*)probs, n_pairs);
    HIP_CHECK(hipGetLastError());
}

// one wave per row
__global__ __launch_bounds__(256) void k_softmax_rows(const float* __restrict__ logits, long ld, int nc, long n,
                                                      float* __restrict__ probs)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* l = logits + row * ld;
    float m = -INFINITY;
    for (int c = lane; c < nc; c += 64) m = fmaxf(m, l[c]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
    for (int c = lane; c < nc; c += 64) sum += expf(l[c] - m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    for (int c = lane; c < nc; c += 64) probs[row * nc + c] = expf(l[c] - m) * inv;
}

void softmax_rows_forward(hipStream_t s, const float* logits, long ld, int nc, long n, float* probs)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, logits, ld, nc, n, probs);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_copy_columns(const float* __restrict__ src, long ld, int c0, int ncols, long n,
                                                      float* __restrict__ dst)
{
    const long total = n * ncols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / ncols;
        const int c = (int)(e - r * ncols);
        dst[e] = src[r * ld + c0 + c];
    }
}

void copy_columns_forward(hipStream_t s, const float* src, long ld, int c0, int ncols, long n, float* dst)
{
    if (n <= 0) return;
    const long total = n * ncols;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(k_copy_columns, dim3(grid), dim3(256), 0, s, src, ld, c0, ncols, n, dst);
    HIP_CHECK(hipGetLastError());
}

// TimeDistributedClassifierLayer.swift:65-86: argmax over all classes (ties → lowest index), score,
// the four deltas of the arg-max class.  One wave per ROI.
// Non-finite rows (a local fp16-range overflow reaches this kernel before the watchdog word is read): NaN entries never win — no comparison
// with a NaN succeeds; a row with no comparable entry (every probability NaN: softmax of a row with a +Inf or NaN logit, or of all -Inf)
// yields class 0, score = the row's probability at index 0 (the NaN as it is) and class 0's deltas, so DetectionLayer drops it
// (score >= threshold is false).  The class index is therefore always inside [0, nc): `bbox` is never read outside the row.
__global__ __launch_bounds__(256) void k_classifier_post(const float* __restrict__ probs, const float* __restrict__ bbox,
                                                         int nc, long n, float* __restrict__ out, long out_row_stride)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = probs + row * nc;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < nc; c += 64) {
        const float v = p[c];
        if (v > bv || (v == bv && c < bi)) { bv = v; bi = c; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) { bi = 0; bv = p[0]; }      // no lane met a comparable entry
    float* o = out + row * out_row_stride;
    if (lane < 4) o[lane] = bbox[row * nc * 4 + (long)bi * 4 + lane];
    else if (lane == 4) o[4] = (float)bi;
    else if (lane == 5) o[5] = bv;
}

void classifier_postprocess_forward(hipStream_t s, const float* probs, const float* bbox, int nc, long n, float* out,
                                    long out_row_stride)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_classifier_post, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, probs, bbox, nc, n, out, out_row_stride);
    HIP_CHECK(hipGetLastError());
}

template <typename T>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const float* __restrict__ in, long n, int C, int HW, T* __restrict__ out)
{
    const long total = n * C * HW;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const int p = (int)((e / C) % HW);
        const long i = e / ((long)C * HW);
        out[e] = (T)in[(i * C + c) * HW + p];
    }
}
__global__ __launch_bounds__(256) void k_nhwc_to_nchw(const float* __restrict__ in, long n, int C, int HW, float* __restrict__ out)
{
    const long total = n * C * HW;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int p = (int)(e % HW);
        const int c = (int)((e / HW) % C);
        const long i = e / ((long)C * HW);
        out[e] = in[(i * HW + p) * C + c];
    }
}
void nchw_to_nhwc_forward(hipStream_t s, const float* in, long n, int C, int H, int W, void* out, int dtype)
{
    const long total = n * C * H * W;
    if (total <= 0) return;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (dtype == MRCNN_F16) hipLaunchKernelGGL(k_nchw_to_nhwc<_Float16>, dim3(grid), dim3(256), 0, s, in, n, C, H * W, (_Float16*)out);
    else hipLaunchKernelGGL(k_nchw_to_nhwc<float>, dim3(grid), dim3(256), 0, s, in, n, C, H * W, (float*)out);
    HIP_CHECK(hipGetLastError());
}
void nhwc_to_nchw_forward(hipStream_t s, const float* in, long n, int C, int H, int W, float* out)
{
    const long total = n * C * H * W;
    if (total <= 0) return;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(grid), dim3(256), 0, s, in, n, C, H * W, out);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_copy_rows(const float* __restrict__ src, long src_stride, long n, long len,
                                                   float* __restrict__ dst, long dst_stride)
{
    const long total = n * len;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / len, c = e - r * len;
        dst[r * dst_stride + c] = src[r * src_stride + c];
    }
}
void copy_rows_forward(hipStream_t s, const float* src, long src_stride, long n, long len, float* dst, long dst_stride)
{
    const long total = n * len;
    if (total <= 0) return;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(k_copy_rows, dim3(grid), dim3(256), 0, s, src, src_stride, n, len, dst, dst_stride);
    HIP_CHECK(hipGetLastError());
}

// ================================================================================================
// TimeDistributedMaskLayer
// ================================================================================================
// MultiArrayBatchProvider(removeZeros:true) (TimeDistributedClassifierLayer.swift:116-127): a row is
// kept iff every element is != 0.
template <typename T>
__global__ __launch_bounds__(256) void k_mask_row_flags(const T* __restrict__ pooled, long pooled_sB, long row_stride,
                                                        long row_len, int ld, int32_t* __restrict__ flags)
{
    const int d = blockIdx.x, b = blockIdx.y;
    const T* r = pooled + (size_t)b * pooled_sB + (size_t)d * row_stride;
    int ok = 1;
    for (long e = threadIdx.x; e < row_len; e += 256) ok &= ((float)r[e] != 0.0f) ? 1 : 0;
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) flags[(size_t)b * ld + d] = ok;
}
__global__ void k_mask_row_compact(const int32_t* __restrict__ flags, int D, int ld, int32_t* __restrict__ mapping,
                                   int32_t* __restrict__ kept)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    int k = 0;
    for (int d = 0; d < D; ++d)
        if (flags[(size_t)b * ld + d]) mapping[(size_t)b * ld + k++] = d;
    kept[b] = k;
}

void mask_valid_rows_forward(hipStream_t s, const void* pooled, long pooled_sB, long row_stride, long row_len, int D,
                             int B, const MaskSelectWorkspace& ws, int dtype)
{
    if (D <= 0 || B <= 0) return;
    const int ld = ws.ld ? ws.ld : D;
    if (!pooled) { /* flags come from the ROIAlign kernel */ }
    else if (dtype == MRCNN_F16)
        hipLaunchKernelGGL(k_mask_row_flags<_Float16>, dim3(D, B), dim3(256), 0, s, (const _Float16*)pooled, pooled_sB, row_stride, row_len, ld, ws.flags);
    else hipLaunchKernelGGL(k_mask_row_flags<float>, dim3(D, B), dim3(256), 0, s, (const float*)pooled, pooled_sB, row_stride, row_len, ld, ws.flags);
    hipLaunchKernelGGL(k_mask_row_compact, dim3(B), dim3(64), 0, s, ws.flags, D, ld, ws.mapping, ws.kept);
    HIP_CHECK(hipGetLastError());
}

// TimeDistributedMaskLayer.swift:58-89 with the Mask model's last layer (1×1 conv to numClasses +
// sigmoid, of which the reference keeps one channel) evaluated for the selected class only.
// Compact index i = blockIdx.y: row actual = mapping[i] is written with class detections[i][4]
// (:71 reads the compact index); rows i >= kept are zero padding (:87-89).
template <typename T>
__global__ __launch_bounds__(256) void k_mask_select(const T* __restrict__ feat, long feat_sB, int HW, int C,
                                                     const float* __restrict__ w, const float* __restrict__ bias, int nc,
                                                     const float* __restrict__ det, long det_sB, long det_stride, int ld,
                                                     const int32_t* __restrict__ mapping, const int32_t* __restrict__ kept,
                                                     float* __restrict__ out, long out_sB, long out_stride)
{
    const int i = blockIdx.y, b = blockIdx.z;
    const int nk = kept[b];
    float* ob = out + (size_t)b * out_sB;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (i >= nk) {
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < out_stride; e += (long)gridDim.x * 256) ob[(size_t)i * out_stride + e] = 0.0f;
        return;
    }
    const int actual = mapping[(size_t)b * ld + i];
    if (actual >= nk) return;                       // would be overwritten by the zero padding
    int cid = (int)det[(size_t)b * det_sB + (size_t)i * det_stride + 4];
    cid = cid < 0 ? 0 : (cid >= nc ? nc - 1 : cid);
    const float* wr = w + (size_t)cid * C;
    const T* f = feat + (size_t)b * feat_sB + (size_t)actual * HW * C;
    for (int p = blockIdx.x * 4 + wave; p < HW; p += gridDim.x * 4) {
        float sum = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 x = load4<T>(f + (size_t)p * C + c);
            const float4 y = *reinterpret_cast<const float4*>(wr + c);
            sum += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) ob[(size_t)actual * out_stride + p] = 1.0f / (1.0f + expf(-(sum + bias[cid])));
    }
    // the reference copies `stride` elements per row (:83); HW == stride for the 28×28 output
}

void mask_select_forward(hipStream_t s, const void* feat, long feat_sB, int HW, int C, const float* w,
                         const float* bias, int nc, const float* det, long det_sB, long det_stride, int D, int B,
                         const MaskSelectWorkspace& ws, float* out, long out_sB, long out_stride, int dtype)
{
    if (D <= 0 || B <= 0) return;
    MRCNN_REQUIRE(C % 4 == 0, MRCNN_ERR_SHAPE, "mask head: C %% 4 != 0");
    if (dtype == MRCNN_F16)
        hipLaunchKernelGGL(k_mask_select<_Float16>, dim3(49, D, B), dim3(256), 0, s, (const _Float16*)feat, feat_sB, HW, C, w, bias, nc, det,
                           det_sB, det_stride, ws.ld ? ws.ld : D, ws.mapping, ws.kept, out, out_sB, out_stride);
    else
        hipLaunchKernelGGL(k_mask_select<float>, dim3(49, D, B), dim3(256), 0, s, (const float*)feat, feat_sB, HW, C, w, bias, nc, det, det_sB,
                           det_stride, ws.ld ? ws.ld : D, ws.mapping, ws.kept, out, out_sB, out_stride);
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// The fused form of the mask head's tail: the deconvolution leaves, per output pixel, `parts` partial dots with the selected
// class's 1x1 filter (conv_epilogue, ConvDesc::sel_partial) instead of its 256-channel fp32 output (642 MB per batch of 8
// that this layer used to read back).  Same control flow as k_mask_select — what TimeDistributedMaskLayer.swift:58-89 writes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_mask_select_classes(const float* __restrict__ det, long det_sB, long det_stride, int D, int ld, int nc,
                                                             const int32_t* __restrict__ mapping, const int32_t* __restrict__ kept,
                                                             int32_t* __restrict__ sel_cid)
{
    const int b = blockIdx.x;
    const int nk = kept[b];
    for (int r = threadIdx.x; r < D; r += blockDim.x) sel_cid[(size_t)b * ld + r] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < nk; i += blockDim.x) {
        const int actual = mapping[(size_t)b * ld + i];
        if (actual >= nk) continue;                     // would be overwritten by the zero padding
        int cid = (int)det[(size_t)b * det_sB + (size_t)i * det_stride + 4];      // the COMPACT index's class (:71)
        cid = cid < 0 ? 0 : (cid >= nc ? nc - 1 : cid);
        sel_cid[(size_t)b * ld + actual] = cid;
    }
}

__global__ __launch_bounds__(256) void k_mask_select_partials(const float* __restrict__ partial, int parts, int HW,
                                                              const float* __restrict__ bias, int D, int ld,
                                                              const int32_t* __restrict__ sel_cid, const int32_t* __restrict__ kept,
                                                              float* __restrict__ out, long out_sB, long out_stride)
{
    const int r = blockIdx.y, b = blockIdx.z;
    const int nk = kept[b];
    float* orow = out + (size_t)b * out_sB + (size_t)r * out_stride;
    const int cid = sel_cid[(size_t)b * ld + r];
    if (r >= nk) {                                       // zero padding (:87-89)
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < out_stride; e += (long)gridDim.x * 256) orow[e] = 0.0f;
        return;
    }
    if (cid < 0) return;                                 // a row the layer never writes
    const float* pr = partial + ((size_t)b * D + r) * HW * parts;
    const float bs = bias[cid];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        float sum = pr[(size_t)p * parts];
        for (int h = 1; h < parts; ++h) sum += pr[(size_t)p * parts + h];
        orow[p] = 1.0f / (1.0f + expf(-(sum + bs)));
    }
}

void mask_select_classes(hipStream_t s, const float* det, long det_sB, long det_stride, int D, int B, int nc,
                         const MaskSelectWorkspace& ws, int32_t* sel_cid)
{
    if (D <= 0 || B <= 0) return;
    hipLaunchKernelGGL(k_mask_select_classes, dim3(B), dim3(128), 0, s, det, det_sB, det_stride, D, ws.ld ? ws.ld : D, nc, ws.mapping, ws.kept, sel_cid);
    HIP_CHECK(hipGetLastError());
}

void mask_select_from_partials(hipStream_t s, const float* partial, int parts, int HW, const float* bias, int nc, const float* det,
                               long det_sB, long det_stride, int D, int B, const MaskSelectWorkspace& ws, float* out, long out_sB,
                               long out_stride)
{
    (void)nc; (void)det; (void)det_sB; (void)det_stride;
    if (D <= 0 || B <= 0) return;
    hipLaunchKernelGGL(k_mask_select_partials, dim3((HW + 255) / 256, D, B), dim3(256), 0, s, partial, parts, HW, bias, D, ws.ld ? ws.ld : D, ws.sel_cid, ws.kept,
                       out, out_sB, out_stride);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_mask_select_full(const float* __restrict__ masks, long masks_sB, int HW, int nc,
                                                          const float* __restrict__ det, long det_sB, long det_stride,
                                                          int ld, const int32_t* __restrict__ mapping,
                                                          const int32_t* __restrict__ kept, float* __restrict__ out,
                                                          long out_sB, long out_stride)
{
    const int i = blockIdx.x, b = blockIdx.y;
    const int nk = kept[b];
    float* ob = out + (size_t)b * out_sB;
    if (i >= nk) {
        for (long e = threadIdx.x; e < out_stride; e += 256) ob[(size_t)i * out_stride + e] = 0.0f;
        return;
    }
    const int actual = mapping[(size_t)b * ld + i];
    if (actual >= nk) return;
    int cid = (int)det[(size_t)b * det_sB + (size_t)i * det_stride + 4];
    cid = cid < 0 ? 0 : (cid >= nc ? nc - 1 : cid);
    const float* src = masks + (size_t)b * masks_sB + ((size_t)actual * nc + cid) * HW;
    for (int e = threadIdx.x; e < HW; e += 256) ob[(size_t)actual * out_stride + e] = src[e];
}

void mask_select_from_full_forward(hipStream_t s, const float* masks, long masks_sB, int HW, int nc, const float* det,
                                   long det_sB, long det_stride, int D, int B, const MaskSelectWorkspace& ws, float* out,
                                   long out_sB, long out_stride)
{
    if (D <= 0 || B <= 0) return;
    hipLaunchKernelGGL(k_mask_select_full, dim3(D, B), dim3(256), 0, s, masks, masks_sB, HW, nc, det, det_sB, det_stride,
                       ws.ld ? ws.ld : D, ws.mapping, ws.kept, out, out_sB, out_stride);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn
