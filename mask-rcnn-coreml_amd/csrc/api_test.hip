// api_test.hip — the C ABI of include/maskrcnn_hip_test.h that is not in probe.hip: the debug knobs, the convolution
// micro-benchmark, single kernels and bottleneck blocks on caller data, the live convolution profile of a model.
#include <string.h>

#include <random>

#include "api_util.h"
#include "conv_pack.h"
#include "knobs.h"

using namespace mrcnn;

// ================================================================================================
// scaffolding of the entries on caller (host) data
// ================================================================================================
namespace {

// host floats -> a device buffer of n_alloc (default n) fp16 / fp32 elements, zero beyond the first n
void upload_f16(DevBuf& d, const float* src, size_t n, size_t n_alloc = 0)
{
    std::vector<_Float16> t(n_alloc > n ? n_alloc : n, (_Float16)0.f);
    for (size_t i = 0; i < n; ++i) t[i] = (_Float16)src[i];
    d.alloc(t.size() * 2);
    HIP_CHECK(hipMemcpy(d.p, t.data(), t.size() * 2, hipMemcpyHostToDevice));
}
void upload_f32(DevBuf& d, const float* src, size_t n, size_t n_alloc = 0)
{
    d.alloc((n_alloc > n ? n_alloc : n) * 4);
    if (n_alloc > n) HIP_CHECK(hipMemset(d.p, 0, n_alloc * 4));
    HIP_CHECK(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice));
}
void download_f16_as_f32(const void* dev, size_t n, float* out)
{
    std::vector<_Float16> t(n);
    HIP_CHECK(hipMemcpy(t.data(), dev, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = (float)t[i];
}

// A K x K convolution (padding K / 2) over dense NHWC tensors; dtype / wdtype / out_f32 are the caller's to set.
ConvDesc dense_nhwc_desc(const void* in, int B, int H, int W, int Cin, const void* wgt, int K, int stride, const float* scale, const float* shift,
                         void* out, int Cout, int Npad, int act)
{
    ConvDesc d;
    d.in = in; d.B = B; d.H = H; d.W = W; d.Cin = Cin;
    d.in_sW = Cin; d.in_sH = (long)W * Cin; d.in_sB = (long)H * W * Cin;
    d.wgt = wgt; d.KH = d.KW = K; d.stride = stride; d.padH = d.padW = K / 2;
    d.scale = scale; d.shift = shift;
    d.OH = (H + 2 * d.padH - K) / stride + 1; d.OW = (W + 2 * d.padW - K) / stride + 1; d.Cout = Cout; d.Npad = Npad;
    d.out = out; d.out_sP = Cout; d.out_sB = (long)d.OH * d.OW * Cout; d.act = act;
    return d;
}
// a dense residual of the output's shape
void set_dense_residual(ConvDesc& d, const void* res)
{
    d.res = res; d.res_sW = d.Cout; d.res_sH = (long)d.OW * d.Cout; d.res_sB = d.out_sB;
}

// A pair of events: the average milliseconds of `iters` calls of run() on a stream.  The events go with the scope, also when a launch throws.
struct EventTimer {
    struct Event {
        hipEvent_t e = nullptr;
        Event() { HIP_CHECK(hipEventCreate(&e)); }
        ~Event() { (void)hipEventDestroy(e); }
    } e0, e1;
    template <class F>
    float avg_ms(hipStream_t s, int iters, F&& run)
    {
        HIP_CHECK(hipEventRecord(e0.e, s));
        for (int i = 0; i < iters; ++i) run();
        HIP_CHECK(hipEventRecord(e1.e, s));
        HIP_CHECK(hipEventSynchronize(e1.e));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
        return ms / iters;
    }
};

// One short-lived ConvScratch for the call (kernels.h), handed to the calling thread's launches until the scope ends
struct ScopedConvScratch {
    ConvScratch scratch;
    explicit ScopedConvScratch(bool wanted) { if (wanted) { scratch.alloc(); conv_set_scratch(&scratch); } }
    ~ScopedConvScratch() { conv_set_scratch(nullptr); }
};

// The fp16-range watchdog word of one entry on caller data (include/maskrcnn_hip_test.h: mrcnn_test_last_range_flag): a 4-byte device flag, zeroed on the
// launch stream, handed to the calling thread's conv_forward launches (watch_conv_family) and, through dev(), to bneck_launch; taken away again however the
// scope ends.  keep() reads the word back into the thread-local the getter returns (0 from the entry's start, so a failed entry never reports a stale word).
thread_local int t_last_range_flag = 0;
struct ScopedRangeFlag {
    DevBuf flag;
    ScopedRangeFlag(hipStream_t s, bool watch_conv_family)
    {
        t_last_range_flag = 0;
        flag.alloc(sizeof(int));
        HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int), s));
        if (watch_conv_family) conv_set_range_flag(flag.as<int>());
    }
    ~ScopedRangeFlag() { conv_set_range_flag(nullptr); }
    int* dev() { return flag.as<int>(); }
    void keep() { HIP_CHECK(hipMemcpy(&t_last_range_flag, flag.p, sizeof(int), hipMemcpyDeviceToHost)); }      // (after the stream has been synchronised)
};

}  // namespace

// ================================================================================================
// convolution micro-benchmark (bench.py roofline leg)
// ================================================================================================
extern "C" int mrcnn_bench_conv(int batch, int h, int w, int cin, int cout, int ksize, int stride, int iters, float* avg_ms,
                                double* flops)
{
    return mrcnn_bench_conv_dtype(batch, h, w, cin, cout, ksize, stride, iters, MRCNN_F32, avg_ms, flops);
}

extern "C" int mrcnn_bench_conv_dtype(int batch, int h, int w, int cin, int cout, int ksize, int stride, int iters, int dtype,
                                      float* avg_ms, double* flops)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(avg_ms && flops && iters >= 1 && (ksize == 1 || ksize == 3) && cin % 64 == 0, MRCNN_ERR_INVALID, "bad bench_conv arguments");
        MRCNN_REQUIRE(dtype == MRCNN_F32 || dtype == MRCNN_F16 || dtype == MRCNN_F32S || dtype == MRCNN_F32X3, MRCNN_ERR_UNSUPPORTED, "bench_conv: dtype %d", dtype);
        const size_t es = dtype == MRCNN_F16 ? 2 : 4;             // activations
        const size_t ws = dtype == MRCNN_F32 ? 4 : 2;             // filters
        const int pad = ksize / 2;
        const int oh = (h + 2 * pad - ksize) / stride + 1, ow = (w + 2 * pad - ksize) / stride + 1;
        const int bn = conv_n_tile(cout), npad = (cout + bn - 1) / bn * bn;
        const size_t n_in = (size_t)batch * h * w * cin, n_w = (size_t)npad * ksize * ksize * cin, n_out = (size_t)batch * oh * ow * cout;
        std::mt19937 rng(7);
        std::uniform_real_distribution<float> U(-1.f, 1.f);
        const std::vector<float> hs(npad, 1.f), hb(npad, 0.f);
        // random operands in [-1,1) (weights scaled); for fp16 the bit patterns are generated directly
        const size_t pat = 1 << 20;
        std::vector<unsigned char> hin(pat * es), hw(n_w * ws);
        auto fill = [&](unsigned char* dst, size_t n, float scale, size_t esz) {
            for (size_t i = 0; i < n; ++i) {
                const float v = U(rng) * scale;
                if (esz == 4) memcpy(dst + i * 4, &v, 4);
                else { const _Float16 hv = (_Float16)v; memcpy(dst + i * 2, &hv, 2); }
            }
        };
        fill(hin.data(), pat, 1.f, es);
        fill(hw.data(), n_w, 0.05f, ws);
        DevBuf din(n_in * es), dw(n_w * ws), ds, db, dout(n_out * es);
        for (size_t off = 0; off < n_in; off += pat) {
            const size_t c = n_in - off < pat ? n_in - off : pat;
            HIP_CHECK(hipMemcpy((char*)din.p + off * es, hin.data(), c * es, hipMemcpyHostToDevice));
        }
        HIP_CHECK(hipMemcpy(dw.p, hw.data(), n_w * ws, hipMemcpyHostToDevice));
        upload_f32(ds, hs.data(), npad);
        upload_f32(db, hb.data(), npad);
        ConvDesc d = dense_nhwc_desc(din.p, batch, h, w, cin, dw.p, ksize, stride, ds.as<float>(), db.as<float>(), dout.p, cout, npad, ACT_RELU);
        d.dtype = (dtype == MRCNN_F32S || dtype == MRCNN_F32X3) ? MRCNN_F32 : dtype;
        d.wdtype = dtype == MRCNN_F32 ? MRCNN_F32 : (dtype == MRCNN_F32X3 ? MRCNN_F32X3 : MRCNN_F16);
        DevBuf dres;
        if (knob_env("MRCNN_BENCH_RESIDUAL") && atoi(knob_env("MRCNN_BENCH_RESIDUAL"))) {        // the bottleneck blocks' branch2c shape
            dres.alloc(n_out * es);
            HIP_CHECK(hipMemset(dres.p, 0, n_out * es));
            set_dense_residual(d, dres.p);
        }
        Stream st;
        DevBuf dwh;
        if (ksize == 3 && ws == 2 && es == 4 && conv_halo_packable(ksize, ksize, cin, npad)) {
            conv_halo_pack(st.s, dw.p, npad, cin, dwh);
            d.wgt_halo = dwh.p;
        }
        DevBuf dw3h;
        if (ws == 2 && es == 2 && stride == 1 && conv3x3h_packable(ksize, ksize, cin, cout, npad)) { conv3x3h_pack(st.s, dw.p, cout, cin, dw3h); d.wgt_c3h = dw3h.p; }
        ScopedConvScratch scratch(ws == 2 && es == 4);      // the split modes' shared-tile K chunks measure as the engine runs them
        EventTimer timer;
        for (int i = 0; i < 2; ++i) conv_forward(st.s, d);   // warm-up, outside the timed region
        *avg_ms = timer.avg_ms(st.s, iters, [&] { conv_forward(st.s, d); });
        *flops = 2.0 * (double)batch * oh * ow * (double)cout * ksize * ksize * cin;
    });
}

// ================================================================================================
// One convolution of the engine's kernel family on caller data (parity tests of the kernels themselves: every tile
// shape / pipeline variant must give bit-identical results, since the choice depends on the batch size)
// ================================================================================================
static int& g_conv2d_alias_res = knob("conv2d_alias_res", nullptr, 0);      // mrcnn_conv2d_nhwc writes its output in place over the residual (tests of the in-place contract)
extern "C" int mrcnn_debug_set(const char* key, int value)
{
    return guarded([&] {
        MRCNN_REQUIRE(key, MRCNN_ERR_INVALID, "null key");
        MRCNN_REQUIRE(test_knobs_armed(), MRCNN_ERR_UNSUPPORTED, "mrcnn_debug_set('%s'): the test / measurement knobs are armed only in a process started with "
                      "MRCNN_TEST_KNOBS=1 (include/maskrcnn_hip_test.h); a production host runs the shipped policy", key);
        MRCNN_REQUIRE(knob_set(key, value), MRCNN_ERR_INVALID, "unknown debug key '%s'", key);
    });
}

extern "C" int mrcnn_conv2d_nhwc(const float* in, int batch, int h, int w, int cin, const float* filters, int cout, int ksize, int stride,
                                 const float* scale, const float* shift, const float* residual, int act, int dtype, float* out)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(in && filters && out && batch >= 1 && h >= 1 && w >= 1 && cout >= 1 && (ksize == 1 || ksize == 3) && stride >= 1,
                      MRCNN_ERR_INVALID, "bad conv2d_nhwc argument");
        MRCNN_REQUIRE(dtype == MRCNN_F32 || dtype == MRCNN_F16 || dtype == MRCNN_F32S || dtype == MRCNN_F32X3, MRCNN_ERR_UNSUPPORTED, "conv2d_nhwc: dtype %d", dtype);
        const int adt = dtype == MRCNN_F16 ? MRCNN_F16 : MRCNN_F32;
        const int wdt = dtype == MRCNN_F32 ? MRCNN_F32 : (dtype == MRCNN_F32X3 ? MRCNN_F32X3 : MRCNN_F16);
        MRCNN_REQUIRE(cin % (adt == MRCNN_F16 ? 64 : 32) == 0, MRCNN_ERR_SHAPE, "conv2d_nhwc: Cin %d not a multiple of the K tile", cin);
        const int pad = ksize / 2;
        const int oh = (h + 2 * pad - ksize) / stride + 1, ow = (w + 2 * pad - ksize) / stride + 1;
        const int bn = conv_n_tile(cout), npad = (cout + bn - 1) / bn * bn;
        const size_t n_in = (size_t)batch * h * w * cin, kk = (size_t)ksize * ksize * cin, n_out = (size_t)batch * oh * ow * cout;
        auto* const upload_act = adt == MRCNN_F16 ? upload_f16 : upload_f32;
        DevBuf din, dw, ds, db, dres, dout;
        upload_act(din, in, n_in, n_in);
        (wdt != MRCNN_F32 ? upload_f16 : upload_f32)(dw, filters, (size_t)cout * kk, (size_t)npad * kk);      // the filter rows up to Npad are zero
        // the padded columns cout..Npad-1 (zero filters) carry a shift far beyond the fp16 range: no epilogue stores them, and one whose watchdog
        // forgot to gate them reports it (tests/test_gpu_range_watch.py)
        std::vector<float> hs(npad, 0.f), hb(npad, 1.0e30f);
        for (int o = 0; o < cout; ++o) { hs[o] = scale ? scale[o] : 1.f; hb[o] = shift ? shift[o] : 0.f; }
        upload_f32(ds, hs.data(), npad);
        upload_f32(db, hb.data(), npad);
        if (residual) upload_act(dres, residual, n_out, n_out);
        dout.alloc(n_out * 4);
        ConvDesc d = dense_nhwc_desc(din.p, batch, h, w, cin, dw.p, ksize, stride, ds.as<float>(), db.as<float>(), dout.p, cout, npad, act);
        d.dtype = adt; d.wdtype = wdt; d.out_f32 = 0;      // fp16 mode stores fp16 (the path the engine's layers take), widened below
        if (residual) set_dense_residual(d, dres.p);
        // mrcnn_debug_set("conv2d_alias_res", 1): the output is written IN PLACE over the residual, the way the engine runs every
        // bottleneck block's branch2c (engine_plan.hip: `to = sc`).  The contract every epilogue must keep (ConvDesc::res in kernels.h):
        // a residual element is loaded by the thread that stores the output element at the same address, before that store.
        if (residual && g_conv2d_alias_res) d.out = dres.p;
        Stream st;
        DevBuf dwh;
        if (ksize == 3 && wdt != MRCNN_F32 && adt == MRCNN_F32 && conv_halo_packable(ksize, ksize, cin, npad)) {
            conv_halo_pack(st.s, dw.p, npad, cin, dwh);
            d.wgt_halo = dwh.p;
        }
        DevBuf dw3h;
        if (adt == MRCNN_F16 && conv3x3h_packable(ksize, ksize, cin, cout, npad)) { conv3x3h_pack(st.s, dw.p, cout, cin, dw3h); d.wgt_c3h = dw3h.p; }
        ScopedConvScratch scratch(wdt != MRCNN_F32 && adt == MRCNN_F32);      // the shared-tile K chunks need it
        ScopedRangeFlag range(st.s, dtype != MRCNN_F32);      // as the engine: the exact-fp32 mode has no fp16 hand-over to watch, its word stays 0
        conv_forward(st.s, d);
        HIP_CHECK(hipStreamSynchronize(st.s));
        range.keep();
        if (adt == MRCNN_F16) download_f16_as_f32(d.out, n_out, out);
        else HIP_CHECK(hipMemcpy(out, d.out, n_out * 4, hipMemcpyDeviceToHost));
    });
}

// One conv_forward of a form only the engine builds (include/maskrcnn_hip_test.h: mrcnn_test_conv_form_nhwc; tests/test_gpu_conv_forms.py): the
// strided input view, the shifted residual, the column split into two pitched outputs, the 2x2 scatter and its selected-class dot, fp32 stores
// of fp16 tensors.  Every output buffer is sentinel-filled and returned whole.
namespace {

// one pitched output of the entry: the device copy of the caller's whole buffer, and where the layer's images sit in it
struct FormOutput {
    DevBuf dev;
    long len = 0, offset = 0, sB = 0, sP = 0, sH = 0;
    bool f32 = true;
    void* base() const { return static_cast<char*>(dev.p) + (size_t)offset * (f32 ? 4 : 2); }
    // cols columns per pixel of a rows x width image; every addressed element must lie inside the buffer
    void lay_out(const mrcnn_test_conv_output& o, const char* who, int B, int rows, int width, int cols, bool deconv, bool as_f32, float sentinel)
    {
        MRCNN_REQUIRE(o.data && o.len > 0 && o.offset >= 0 && o.pitch >= 0 && o.row_pitch >= 0 && o.batch_stride >= 0, MRCNN_ERR_INVALID, "test_conv_form: output %s missing or negative", who);
        MRCNN_REQUIRE(deconv || o.row_pitch == 0, MRCNN_ERR_INVALID, "test_conv_form: output %s: a row pitch goes with deconv2 only (rows of an image are contiguous)", who);
        len = o.len; offset = o.offset; f32 = as_f32;
        sP = o.pitch ? o.pitch : cols;
        sH = o.row_pitch ? o.row_pitch : (long)width * sP;
        MRCNN_REQUIRE(sP >= cols && sH >= (long)width * sP, MRCNN_ERR_SHAPE, "test_conv_form: output %s: pitch %ld under %d columns, or row pitch %ld under a row", who, sP, cols, sH);
        const long image = (long)(rows - 1) * sH + (long)(width - 1) * sP + cols;      // the elements from an image's first to its last addressed one
        sB = o.batch_stride ? o.batch_stride : (long)rows * sH;
        MRCNN_REQUIRE(sB >= (long)rows * sH, MRCNN_ERR_SHAPE, "test_conv_form: output %s: batch stride %ld under an image of %ld", who, sB, (long)rows * sH);
        MRCNN_REQUIRE(offset + (long)(B - 1) * sB + image <= len, MRCNN_ERR_SHAPE, "test_conv_form: output %s: %d images do not fit %ld elements behind offset %ld", who, B, len, offset);
        const std::vector<float> fill((size_t)len, sentinel);
        (f32 ? upload_f32 : upload_f16)(dev, fill.data(), fill.size(), 0);
    }
    void deliver(float* dst) const
    {
        if (f32) HIP_CHECK(hipMemcpy(dst, dev.p, (size_t)len * 4, hipMemcpyDeviceToHost));
        else download_f16_as_f32(dev.p, (size_t)len, dst);
    }
};

}  // namespace

extern "C" int mrcnn_test_conv_form_nhwc(const mrcnn_test_conv_form* form)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(form, MRCNN_ERR_INVALID, "test_conv_form: null form");
        const mrcnn_test_conv_form& f = *form;
        const int dtype = f.dtype, B = f.batch, H = f.h, W = f.w, Cin = f.cin, Cout = f.cout, K = f.ksize;
        MRCNN_REQUIRE(f.in && f.filters && B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && (K == 1 || K == 3) && f.stride >= 1 && f.act >= 0 && f.act <= 2,
                      MRCNN_ERR_INVALID, "bad test_conv_form argument");
        MRCNN_REQUIRE(dtype == MRCNN_F32 || dtype == MRCNN_F16 || dtype == MRCNN_F32S || dtype == MRCNN_F32X3, MRCNN_ERR_UNSUPPORTED, "test_conv_form: dtype %d", dtype);
        MRCNN_REQUIRE((f.in_step == 1 || f.in_step == 2) && (f.res_shift == 0 || f.res_shift == 1) && (f.deconv2 == 0 || f.deconv2 == 1) && (f.out_f32 == 0 || f.out_f32 == 1),
                      MRCNN_ERR_INVALID, "test_conv_form: in_step 1 | 2, res_shift / deconv2 / out_f32 0 | 1");
        const bool sel = f.sel_w != nullptr;
        MRCNN_REQUIRE(!f.out_f32 || dtype == MRCNN_F16, MRCNN_ERR_INVALID, "test_conv_form: out_f32 is an option of MRCNN_F16 (the other modes store fp32 anyway)");
        MRCNN_REQUIRE(f.res_shift == 0 || f.residual, MRCNN_ERR_INVALID, "test_conv_form: res_shift without a residual");
        MRCNN_REQUIRE(f.n_split >= 0 && f.n_split < Cout, MRCNN_ERR_INVALID, "test_conv_form: n_split %d outside [0, cout %d)", f.n_split, Cout);
        MRCNN_REQUIRE(!f.deconv2 || (K == 1 && f.stride == 1 && f.in_step == 1 && !f.residual && f.n_split == 0), MRCNN_ERR_INVALID,
                      "test_conv_form: deconv2 is a 1x1 stride-1 GEMM over a dense input with one output and no residual");
        MRCNN_REQUIRE(!sel || (f.deconv2 && f.sel_cid && f.sel_partial && f.sel_parts && f.nc >= 1), MRCNN_ERR_INVALID,
                      "test_conv_form: the selected-class mode needs deconv2, sel_cid, nc >= 1 and somewhere to put the partial sums");
        const int adt = dtype == MRCNN_F16 ? MRCNN_F16 : MRCNN_F32;
        const int wdt = dtype == MRCNN_F32 ? MRCNN_F32 : (dtype == MRCNN_F32X3 ? MRCNN_F32X3 : MRCNN_F16);
        MRCNN_REQUIRE(Cin % (adt == MRCNN_F16 ? 64 : 32) == 0, MRCNN_ERR_SHAPE, "test_conv_form: Cin %d not a multiple of the K tile", Cin);
        const bool half = adt == MRCNN_F16;
        auto* const upload_act = half ? upload_f16 : upload_f32;
        const int ncols = f.deconv2 ? 4 * Cout : Cout;
        const int bn = conv_n_tile(ncols), npad = (ncols + bn - 1) / bn * bn;
        const int step = f.in_step;

        // the input: dense (B, H*step, W*step, Cin), read through strides
        DevBuf din, dw, ds, db, dres, dselw, dcid, dpartial;
        const size_t n_in = (size_t)B * (H * step) * (W * step) * Cin;
        upload_act(din, f.in, n_in, n_in);
        // the filters, in conv_pack.h's layouts; the padded rows are zero ...
        const std::vector<float> wp = f.deconv2 ? pack_deconv2_rows(Cin, Cout, npad, [&](int dy, int dx, int o, int i) { return f.filters[(((size_t)dy * 2 + dx) * Cout + o) * Cin + i]; })
                                                : pack_filter_rows(Cout, Cin, K, K, npad, [&](int o, int y, int x, int i) { return f.filters[(((size_t)o * K + y) * K + x) * Cin + i]; });
        (wdt != MRCNN_F32 ? upload_f16 : upload_f32)(dw, wp.data(), wp.size(), 0);
        // ... and carry a shift far beyond the fp16 range, as in mrcnn_conv2d_nhwc: no epilogue stores them, and a watchdog that forgot to gate them reports it
        std::vector<float> hs(npad, 0.f), hb(npad, 1.0e30f);
        for (int q = 0; q < (f.deconv2 ? 4 : 1); ++q)
            for (int o = 0; o < Cout; ++o) {
                const int n = f.deconv2 ? deconv2_row(q >> 1, q & 1, o, Cout) : o;
                hs[n] = f.scale ? f.scale[o] : 1.f; hb[n] = f.shift ? f.shift[o] : 0.f;
            }
        upload_f32(ds, hs.data(), npad);
        upload_f32(db, hb.data(), npad);

        ConvDesc d = dense_nhwc_desc(din.p, B, H, W, Cin, dw.p, K, f.stride, ds.as<float>(), db.as<float>(), nullptr, Cout, npad, f.act);
        d.in_sW = (long)step * Cin; d.in_sH = (long)step * (W * step) * Cin; d.in_sB = (long)(H * step) * (W * step) * Cin;
        d.dtype = adt; d.wdtype = wdt; d.out_f32 = f.out_f32;
        const int OH = d.OH, OW = d.OW;
        if (f.residual) {
            const int RH = f.res_shift ? (OH + 1) / 2 : OH, RW = f.res_shift ? (OW + 1) / 2 : OW;
            const size_t n_res = (size_t)B * RH * RW * Cout;
            upload_act(dres, f.residual, n_res, n_res);
            d.res = dres.p; d.res_sW = Cout; d.res_sH = (long)RW * Cout; d.res_sB = (long)RH * RW * Cout; d.res_shift = f.res_shift;
        }
        // the outputs
        const bool st32 = !half || f.out_f32;
        FormOutput o1, o2;
        if (!sel) {
            o1.lay_out(f.out, "out", B, f.deconv2 ? 2 * H : OH, f.deconv2 ? 2 * W : OW, f.n_split ? f.n_split : Cout, f.deconv2 != 0, st32, f.sentinel);
            d.out = o1.base(); d.out_sB = o1.sB; d.out_sP = o1.sP;
            if (f.deconv2) { d.deconv2 = 1; d.out_sH = o1.sH; d.out_sW = o1.sP; }
        }
        if (f.n_split) {
            o2.lay_out(f.out2, "out2", B, OH, OW, Cout - f.n_split, false, st32, f.sentinel);
            d.out2 = o2.base(); d.out2_sB = o2.sB; d.out2_sP = o2.sP; d.n_split = f.n_split;
        }
        size_t n_partial = 0;
        if (sel) {
            for (int b = 0; b < B; ++b) MRCNN_REQUIRE(f.sel_cid[b] < f.nc, MRCNN_ERR_INVALID, "test_conv_form: sel_cid[%d] = %d with %d classes", b, f.sel_cid[b], f.nc);
            MRCNN_REQUIRE(Cout % conv_sel_part_cols() == 0, MRCNN_ERR_SHAPE, "test_conv_form: cout %d is not a multiple of the %d-column partial sums", Cout, conv_sel_part_cols());
            *f.sel_parts = Cout / conv_sel_part_cols();
            n_partial = (size_t)B * 4 * H * W * *f.sel_parts;
            const std::vector<float> fill(n_partial, f.sentinel);
            upload_f32(dpartial, fill.data(), n_partial);
            upload_f32(dselw, f.sel_w, (size_t)f.nc * Cout);
            dcid.alloc((size_t)B * 4);
            HIP_CHECK(hipMemcpy(dcid.p, f.sel_cid, (size_t)B * 4, hipMemcpyHostToDevice));
            // (`out` is not written in this mode; the description keeps the scatter's strides of a dense image, as the engine's does)
            d.deconv2 = 1; d.out_sP = Cout; d.out_sW = Cout; d.out_sH = (long)2 * W * Cout; d.out_sB = (long)4 * H * W * Cout;
            d.sel_w = dselw.as<float>(); d.sel_cid = dcid.as<int32_t>(); d.sel_partial = dpartial.as<float>();
        }
        Stream st;
        DevBuf dwh;
        if (K == 3 && wdt != MRCNN_F32 && !half && conv_halo_packable(K, K, Cin, npad)) {
            conv_halo_pack(st.s, dw.p, npad, Cin, dwh);
            d.wgt_halo = dwh.p;
        }
        ScopedConvScratch scratch(wdt != MRCNN_F32 && !half);
        ScopedRangeFlag range(st.s, dtype != MRCNN_F32);
        conv_forward(st.s, d);
        HIP_CHECK(hipStreamSynchronize(st.s));
        range.keep();
        if (!sel) o1.deliver(f.out.data);
        if (f.n_split) o2.deliver(f.out2.data);
        if (sel) HIP_CHECK(hipMemcpy(f.sel_partial, dpartial.p, n_partial * 4, hipMemcpyDeviceToHost));
    });
}

// An identity bottleneck block of the fp16 mode on caller (host) data — the unit tests/test_gpu_bneck.py compares bit for bit:
// fused = 1: the single persistent launch (kernels_bneck.hip); 0: the three launches of the 128-row / ping-pong kernels.
extern "C" int mrcnn_bottleneck_nhwc(const float* x, int batch, int h, int w, int cmid, const float* w1, const float* w2, const float* w3,
                                     const float* s1, const float* h1, const float* s2, const float* h2, const float* s3, const float* h3,
                                     int fused, int iters, float* out, float* avg_ms)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(x && w1 && w2 && w3 && s1 && h1 && s2 && h2 && s3 && h3 && out && batch >= 1 && h >= 1 && w >= 1 && cmid >= 64 && cmid % 64 == 0,
                      MRCNN_ERR_INVALID, "bad bottleneck_nhwc argument");
        const int C = cmid, C4 = 4 * cmid;
        const size_t npix = (size_t)batch * h * w;
        DevBuf dx, dy, dt1, dt2, dw1, dw2, dw3, ds1, dh1, ds2, dh2, ds3, dh3;
        upload_f16(dx, x, npix * C4);
        upload_f16(dw1, w1, (size_t)C * C4);
        upload_f16(dw2, w2, (size_t)C * 9 * C);
        upload_f16(dw3, w3, (size_t)C4 * C);
        upload_f32(ds1, s1, C); upload_f32(dh1, h1, C); upload_f32(ds2, s2, C); upload_f32(dh2, h2, C); upload_f32(ds3, s3, C4); upload_f32(dh3, h3, C4);
        dy.alloc(npix * C4 * 2); dt1.alloc(npix * C * 2); dt2.alloc(npix * C * 2);
        HIP_CHECK(hipMemset(dy.p, 0xff, npix * C4 * 2));
        auto desc = [&](const void* in, int cin, const void* wgt, int k, const float* sc, const float* sh, void* o, int cout) {
            ConvDesc d = dense_nhwc_desc(in, batch, h, w, cin, wgt, k, 1, sc, sh, o, cout, cout, ACT_RELU);
            d.dtype = d.wdtype = MRCNN_F16;
            return d;
        };
        ConvDesc da = desc(dx.p, C4, dw1.p, 1, ds1.as<float>(), dh1.as<float>(), dt1.p, C);
        ConvDesc db = desc(dt1.p, C, dw2.p, 3, ds2.as<float>(), dh2.as<float>(), dt2.p, C);
        ConvDesc dc = desc(dt2.p, C, dw3.p, 1, ds3.as<float>(), dh3.as<float>(), dy.p, C4);
        set_dense_residual(dc, dx.p);
        Stream st;
        DevBuf dw1f, dw2f, dw3f;
        if (bneck_frag_wanted(1, 1, C4, C)) { bneck_pack_frag(st.s, dw1.p, C, C4, dw1f); da.wgt_frag = dw1f.p; }
        if (bneck_frag_wanted(3, 3, C, C)) { bneck_pack_frag(st.s, dw2.p, C, 9 * C, dw2f); db.wgt_frag = dw2f.p; }
        if (bneck_frag_wanted(1, 1, C, C4)) { bneck_pack_frag(st.s, dw3.p, C4, C, dw3f); dc.wgt_frag = dw3f.p; }
        MRCNN_REQUIRE(!fused || conv_bneck_fusable(da, db, dc), MRCNN_ERR_UNSUPPORTED, "bottleneck_nhwc: C %d at %dx%d does not qualify for the fused launch", C, h, w);
        ScopedRangeFlag range(st.s, true);
        auto run = [&] {
            if (fused) {        // the fused launch whatever the grid size (conv_bneck_forward sends under-filled grids to the three launches)
                bneck_launch(st.s, C, da.in, dc.out, batch, h, w, da.wgt, db.wgt, dc.wgt, da.scale, da.shift, db.scale, db.shift, dc.scale, dc.shift, range.dev(), device_cu_count(),
                             fused == 2 ? nullptr : db.wgt_frag, fused == 2 ? nullptr : dc.wgt_frag, fused == 2 ? nullptr : da.wgt_frag);
            }
            else { conv_forward(st.s, da); conv_forward(st.s, db); conv_forward(st.s, dc); }
        };
        run();
        HIP_CHECK(hipStreamSynchronize(st.s));
        range.keep();      // the word of the first run (the timed repeats below see the same data)
        if (iters > 0 && avg_ms) *avg_ms = EventTimer().avg_ms(st.s, iters, run);
        download_f16_as_f32(dy.p, npix * C4, out);
    });
}

// A chained pair of the split modes on caller (host) data (kernels_conv_chain.hip): P = branch2c (t2 -> y, + residual x or the shortcut convolution
// ws of xs, ReLU) and Q = the next block's branch2a (y -> t1, ReLU).  chained = 1: the one launch whatever the grid size; 0: the two launches.
// tests/test_gpu_conv_chain.py compares them bit for bit.
extern "C" int mrcnn_conv_chain_nhwc(const float* t2, int batch, int h, int w, int cmid, const float* w3, const float* s3, const float* h3, const float* x,
                                     const float* xs, int cs, int ss, const float* ws, const float* s_s, const float* h_s,
                                     const float* w1, const float* s1, const float* h1, int dtype, int chained, int in_place, float* y, float* t1)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(t2 && w3 && s3 && h3 && w1 && s1 && h1 && y && t1 && batch >= 1 && h >= 1 && w >= 1 && cmid >= 32 && cmid % 32 == 0, MRCNN_ERR_INVALID, "bad conv_chain_nhwc argument");
        MRCNN_REQUIRE((x != nullptr) != (xs != nullptr), MRCNN_ERR_INVALID, "conv_chain_nhwc: either the residual x or the shortcut's input xs");
        MRCNN_REQUIRE(!xs || (ws && s_s && h_s && cs >= 32 && cs % 32 == 0 && ss >= 1), MRCNN_ERR_INVALID, "conv_chain_nhwc: the shortcut's operands");
        MRCNN_REQUIRE(dtype == MRCNN_F32S || dtype == MRCNN_F32X3, MRCNN_ERR_UNSUPPORTED, "conv_chain_nhwc: dtype %d (split modes only)", dtype);
        const int C = cmid, C4 = 4 * cmid;
        const int wdt = dtype == MRCNN_F32X3 ? MRCNN_F32X3 : MRCNN_F16;
        const size_t npix = (size_t)batch * h * w;
        DevBuf dt2, dw3, ds3, dh3, dx, dxs, dws, dss, dhs, dw1, ds1, dh1, dy, dt1;
        upload_f32(dt2, t2, npix * C);
        upload_f16(dw3, w3, (size_t)C4 * C); upload_f32(ds3, s3, C4); upload_f32(dh3, h3, C4);
        upload_f16(dw1, w1, (size_t)C * C4); upload_f32(ds1, s1, C); upload_f32(dh1, h1, C);
        dx.alloc(npix * C4 * 4);          // the residual: the caller's x, or the shortcut tensor of the two-launch form
        if (x) HIP_CHECK(hipMemcpy(dx.p, x, npix * C4 * 4, hipMemcpyHostToDevice));
        else {
            HIP_CHECK(hipMemset(dx.p, 0xff, npix * C4 * 4));
            upload_f32(dxs, xs, (size_t)batch * (h * ss) * (w * ss) * cs);
            upload_f16(dws, ws, (size_t)C4 * cs); upload_f32(dss, s_s, C4); upload_f32(dhs, h_s, C4);
        }
        // C = 256: both filters also as stream images, packed by the engine's own routine (csrc/conv_pack.h)
        DevBuf dw3s, dw1s;
        if (C == 256) {
            auto stream = [&](DevBuf& d, const float* src, bool q) {
                std::vector<_Float16> hw((size_t)C4 * C);
                for (size_t i = 0; i < hw.size(); ++i) hw[i] = (_Float16)src[i];
                const std::vector<_Float16> img = pack_chain_stream(hw.data(), C, q);
                d.alloc(img.size() * 2);
                HIP_CHECK(hipMemcpy(d.p, img.data(), img.size() * 2, hipMemcpyHostToDevice));
            };
            stream(dw3s, w3, false);
            stream(dw1s, w1, true);
        }
        dy.alloc(npix * C4 * 4); dt1.alloc(npix * C * 4);
        HIP_CHECK(hipMemset(dy.p, 0xff, npix * C4 * 4));
        HIP_CHECK(hipMemset(dt1.p, 0xff, npix * C * 4));
        void* const yout = in_place ? dx.p : dy.p;
        auto desc = [&](const void* in, int hh, int ww, int cin, const void* wgt, int stride, const float* sc, const float* sh, void* o, int cout, int act) {
            ConvDesc d = dense_nhwc_desc(in, batch, hh, ww, cin, wgt, 1, stride, sc, sh, o, cout, cout, act);
            d.dtype = MRCNN_F32; d.wdtype = wdt;
            return d;
        };
        ConvDesc dP = desc(dt2.p, h, w, C, dw3.p, 1, ds3.as<float>(), dh3.as<float>(), yout, C4, ACT_RELU);
        set_dense_residual(dP, dx.p);
        ConvDesc dQ = desc(yout, h, w, C4, dw1.p, 1, ds1.as<float>(), dh1.as<float>(), dt1.p, C, ACT_RELU);
        dP.wgt_stream = dw3s.p; dQ.wgt_stream = dw1s.p;
        ConvDesc dS;
        if (xs) dS = desc(dxs.p, h * ss, w * ss, cs, dws.p, ss, dss.as<float>(), dhs.as<float>(), dx.p, C4, ACT_NONE);
        MRCNN_REQUIRE(!xs || (dS.OH == h && dS.OW == w), MRCNN_ERR_SHAPE, "conv_chain_nhwc: the shortcut's output is not %d x %d", h, w);
        MRCNN_REQUIRE(!chained || conv_chain_fusable(dP, dQ, xs ? &dS : nullptr), MRCNN_ERR_UNSUPPORTED, "conv_chain_nhwc: C %d at %dx%d does not qualify for the chained launch", C, h, w);
        // the policy knob for the length of the call: 3 = chained at every grid size, the shortcut riding too; 0 = the two launches
        struct ScopedKnob {
            std::vector<std::pair<int*, int>> saved;
            ScopedKnob(const char* key, int v) { const auto r = knob_table().by_key.equal_range(key); for (auto it = r.first; it != r.second; ++it) { saved.emplace_back(it->second, *it->second); *it->second = v; } }
            ~ScopedKnob() { for (auto& kv : saved) *kv.first = kv.second; }
        } knob_scope("conv_chain", chained ? 3 : 0), knob_scope4("conv_chain4", chained ? 2 : 0);          // (C = 256 has its own knob)
        Stream st;
        ScopedConvScratch scratch(true);
        ScopedRangeFlag range(st.s, true);
        conv_forward_chain(st.s, dP, dQ, xs ? &dS : nullptr);
        HIP_CHECK(hipStreamSynchronize(st.s));
        range.keep();
        HIP_CHECK(hipMemcpy(y, yout, npix * C4 * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(t1, dt1.p, npix * C * 4, hipMemcpyDeviceToHost));
    });
}

// The stream image of one filter of a chainable C = 256 pair, as the engine and mrcnn_conv_chain_nhwc pack it (csrc/conv_pack.h; host only).
extern "C" int mrcnn_test_chain_stream_image(const float* w, int cmid, int q, uint16_t* image)
{
    return guarded([&] {
        MRCNN_REQUIRE(w && image && cmid == 256, MRCNN_ERR_INVALID, "bad chain_stream_image argument");
        std::vector<_Float16> hw((size_t)4 * cmid * cmid);
        for (size_t i = 0; i < hw.size(); ++i) hw[i] = (_Float16)w[i];
        const std::vector<_Float16> img = pack_chain_stream(hw.data(), cmid, q != 0);
        memcpy(image, img.data(), img.size() * 2);
    });
}

// The stage-entry block (res2a of the fp16 mode: x (B,H,W,C) -> (B,H,W,4C), shortcut = the 1x1 convolution ws of x) — fused = 1: one launch
// (kernels_bneck.hip, FIRST form); 0: the four launches.  tests/test_gpu_bneck.py compares them bit for bit.
extern "C" int mrcnn_bottleneck_first_nhwc(const float* x, int batch, int h, int w, int cmid, const float* w1, const float* w2, const float* w3, const float* ws,
                                           const float* const bn[8], int fused, int iters, float* out, float* avg_ms)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(x && w1 && w2 && w3 && ws && bn && out && batch >= 1 && h >= 1 && w >= 1 && cmid >= 64 && cmid % 64 == 0, MRCNN_ERR_INVALID, "bad bottleneck_first_nhwc argument");
        const int C = cmid, C4 = 4 * cmid;
        const size_t npix = (size_t)batch * h * w;
        DevBuf dx, dy, dsc, dt1, dt2, dw1, dw2, dw3, dws, dbn[8];
        upload_f16(dx, x, npix * C);
        upload_f16(dw1, w1, (size_t)C * C); upload_f16(dw2, w2, (size_t)C * 9 * C); upload_f16(dw3, w3, (size_t)C4 * C); upload_f16(dws, ws, (size_t)C4 * C);
        const int bn_n[8] = {C, C, C, C, C4, C4, C4, C4};
        for (int i = 0; i < 8; ++i) upload_f32(dbn[i], bn[i], (size_t)bn_n[i]);
        dy.alloc(npix * C4 * 2); dsc.alloc(npix * C4 * 2); dt1.alloc(npix * C * 2); dt2.alloc(npix * C * 2);
        HIP_CHECK(hipMemset(dy.p, 0xff, npix * C4 * 2));
        auto desc = [&](const void* in, int cin, const void* wgt, int k, int bi, void* o, int cout, int act) {
            ConvDesc d = dense_nhwc_desc(in, batch, h, w, cin, wgt, k, 1, dbn[bi].as<float>(), dbn[bi + 1].as<float>(), o, cout, cout, act);
            d.dtype = d.wdtype = MRCNN_F16;
            return d;
        };
        ConvDesc da = desc(dx.p, C, dw1.p, 1, 0, dt1.p, C, ACT_RELU);
        ConvDesc db = desc(dt1.p, C, dw2.p, 3, 2, dt2.p, C, ACT_RELU);
        ConvDesc dc = desc(dt2.p, C, dw3.p, 1, 4, dy.p, C4, ACT_RELU);
        ConvDesc ds = desc(dx.p, C, dws.p, 1, 6, dsc.p, C4, ACT_NONE);
        set_dense_residual(dc, dsc.p);
        MRCNN_REQUIRE(!fused || conv_bneck_first_fusable(da, db, dc, ds), MRCNN_ERR_UNSUPPORTED, "bottleneck_first_nhwc: C %d at %dx%d does not qualify for the fused launch", C, h, w);
        Stream st;
        ScopedRangeFlag range(st.s, true);
        auto run = [&] {
            if (fused) bneck_launch(st.s, C, da.in, dc.out, batch, h, w, da.wgt, db.wgt, dc.wgt, da.scale, da.shift, db.scale, db.shift, dc.scale, dc.shift, range.dev(), device_cu_count(),
                                    nullptr, nullptr, nullptr, ds.wgt, ds.scale, ds.shift);
            else { conv_forward(st.s, da); conv_forward(st.s, ds); conv_forward(st.s, db); conv_forward(st.s, dc); }
        };
        run();
        HIP_CHECK(hipStreamSynchronize(st.s));
        range.keep();
        if (iters > 0 && avg_ms) *avg_ms = EventTimer().avg_ms(st.s, iters, run);
        download_f16_as_f32(dy.p, npix * C4, out);
    });
}

// The identity blocks of a C = 256 stage on caller data (tests/test_gpu_bneck.py): nlayers blocks with stacked operands — w1 (n,C,4C), w2 (n,C,3,3,C),
// w3 (n,4C,C), bn[6] = s1,h1,s2,h2 (n,C) and s3,h3 (n,4C).  form 1: ONE launch (kernels_bneck.hip, STAGE form: tiles wait for their neighbours' previous
// block); form 0: one fused launch per block.  out = the last block's output.  status_flag (optional) receives the launch's flag word (bit 1: no progress).
extern "C" int mrcnn_bottleneck_stage_nhwc(const float* x, int batch, int h, int w, int nlayers, const float* w1, const float* w2, const float* w3,
                                           const float* const bn[6], int form, int iters, float* out, float* avg_ms, int* status_flag)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(x && w1 && w2 && w3 && bn && out && batch >= 1 && h >= 1 && w >= 1 && nlayers >= 1, MRCNN_ERR_INVALID, "bad bottleneck_stage_nhwc argument");
        const int C = 256, C4 = 1024;
        MRCNN_REQUIRE(bneck_geometry_ok(C, h, w), MRCNN_ERR_UNSUPPORTED, "bottleneck_stage_nhwc: %dx%d does not qualify", h, w);
        const size_t npix = (size_t)batch * h * w;
        DevBuf dx, dx0, dy, dbn[6], flag;
        upload_f16(dx0, x, npix * C4);
        dx.alloc(npix * C4 * 2); dy.alloc(npix * C4 * 2);
        flag.alloc(sizeof(int));
        const size_t bn_n[6] = {(size_t)C, (size_t)C, (size_t)C, (size_t)C, (size_t)C4, (size_t)C4};
        for (int i = 0; i < 6; ++i) upload_f32(dbn[i], bn[i], bn_n[i] * nlayers);
        Stream st;
        std::vector<DevBuf> dw(3 * (size_t)nlayers), df(3 * (size_t)nlayers);
        const size_t rb = bneck_layer_record_bytes();
        std::vector<unsigned char> recs(rb * nlayers);
        for (int l = 0; l < nlayers; ++l) {
            upload_f16(dw[3 * l], w1 + (size_t)l * C * C4, (size_t)C * C4);
            upload_f16(dw[3 * l + 1], w2 + (size_t)l * C * 9 * C, (size_t)C * 9 * C);
            upload_f16(dw[3 * l + 2], w3 + (size_t)l * C4 * C, (size_t)C4 * C);
            bneck_pack_frag(st.s, dw[3 * l].p, C, C4, df[3 * l]);
            bneck_pack_frag(st.s, dw[3 * l + 1].p, C, 9 * C, df[3 * l + 1]);
            bneck_pack_frag(st.s, dw[3 * l + 2].p, C4, C, df[3 * l + 2]);
            bneck_layer_record(recs.data() + l * rb, df[3 * l].p, df[3 * l + 1].p, df[3 * l + 2].p, dbn[0].as<float>() + (size_t)l * C, dbn[1].as<float>() + (size_t)l * C,
                               dbn[2].as<float>() + (size_t)l * C, dbn[3].as<float>() + (size_t)l * C, dbn[4].as<float>() + (size_t)l * C4, dbn[5].as<float>() + (size_t)l * C4);
        }
        const int ntiles = batch * (h / 8) * (w / 16);
        DevBuf tab(recs.size() + (size_t)ntiles * sizeof(unsigned));
        HIP_CHECK(hipMemcpy(tab.p, recs.data(), recs.size(), hipMemcpyHostToDevice));
        unsigned* const done = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(tab.p) + recs.size());
        const int n_cus = device_cu_count();
        auto run = [&] {
            HIP_CHECK(hipMemcpyAsync(dx.p, dx0.p, npix * C4 * 2, hipMemcpyDeviceToDevice, st.s));      // (the blocks overwrite the input tensor from the second one on)
            HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int), st.s));
            if (form == 1) bneck_stage_launch(st.s, tab.p, nlayers, dx.p, dy.p, batch, h, w, done, flag.as<int>(), n_cus);
            else
                for (int l = 0; l < nlayers; ++l) {
                    void* const pi = (l & 1) ? dy.p : dx.p;
                    void* const po = (l & 1) ? dx.p : dy.p;
                    bneck_launch(st.s, C, pi, po, batch, h, w, dw[3 * l].p, dw[3 * l + 1].p, dw[3 * l + 2].p, dbn[0].as<float>() + (size_t)l * C, dbn[1].as<float>() + (size_t)l * C,
                                 dbn[2].as<float>() + (size_t)l * C, dbn[3].as<float>() + (size_t)l * C, dbn[4].as<float>() + (size_t)l * C4, dbn[5].as<float>() + (size_t)l * C4,
                                 flag.as<int>(), n_cus, df[3 * l + 1].p, df[3 * l + 2].p, df[3 * l].p);
                }
        };
        run();
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (status_flag) HIP_CHECK(hipMemcpy(status_flag, flag.p, sizeof(int), hipMemcpyDeviceToHost));
        if (iters > 0 && avg_ms) *avg_ms = EventTimer().avg_ms(st.s, iters, run);      // (includes the input copy and the two memsets of a run: the same for both forms)
        download_f16_as_f32((nlayers & 1) ? dy.p : dx.p, npix * C4, out);
    });
}

extern "C" int mrcnn_test_last_range_flag(int* flag)
{
    return guarded([&] {
        MRCNN_REQUIRE(flag, MRCNN_ERR_INVALID, "null flag");
        *flag = t_last_range_flag;
    });
}

// softmax_rows_forward + classifier_postprocess_forward on caller rows: what ClassifierHead::forward runs behind its last inner product
// (logits at the padded row stride ld of the stacked logits + deltas tensor).
extern "C" int mrcnn_classifier_rows(const float* logits, int64_t ld, const float* bbox, int nc, int64_t n, float* probs_out, float* cls6_out)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(logits && bbox && probs_out && cls6_out && nc >= 1 && ld >= nc && n >= 1, MRCNN_ERR_INVALID, "bad classifier_rows argument");
        DevBuf dl, db, dp, dc;
        upload_f32(dl, logits, (size_t)n * ld);
        upload_f32(db, bbox, (size_t)n * nc * 4);
        dp.alloc((size_t)n * nc * 4);
        dc.alloc((size_t)n * 6 * 4);
        Stream st;
        softmax_rows_forward(st.s, dl.as<float>(), ld, nc, n, dp.as<float>());
        classifier_postprocess_forward(st.s, dp.as<float>(), db.as<float>(), nc, n, dc.as<float>(), 6);
        HIP_CHECK(hipStreamSynchronize(st.s));
        HIP_CHECK(hipMemcpy(probs_out, dp.p, (size_t)n * nc * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cls6_out, dc.p, (size_t)n * 6 * 4, hipMemcpyDeviceToHost));
    });
}

// roi_align_forward (NHWC) on a BATCH of caller (host) data with per-level multipliers — the two things mrcnn_roi_align_nhwc cannot reach: the batch strides
// of the maps, the ROIs, the output and the flags, and PyramidMaps::mul (tests/test_gpu_roi_align_nhwc.py).
extern "C" int mrcnn_test_roi_align_nhwc_batch(const float* const maps[4], const int heights[4], const int widths[4], int channels, int dtype,
                                               const float level_mul[4], const float* rois, int64_t roi_stride, int n_rois, int batch, int pool,
                                               double image_w, double image_h, float* out, int32_t* row_flags)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(maps && heights && widths && level_mul && rois && out, MRCNN_ERR_INVALID, "null argument");
        MRCNN_REQUIRE(dtype == MRCNN_F32 || dtype == MRCNN_F16, MRCNN_ERR_UNSUPPORTED, "test_roi_align_nhwc_batch: dtype %d", dtype);
        MRCNN_REQUIRE(n_rois >= 1 && batch >= 1 && pool >= 1 && channels >= 4 && channels % 4 == 0 && roi_stride >= 4, MRCNN_ERR_INVALID,
                      "bad test_roi_align_nhwc_batch argument");
        const bool f16 = dtype == MRCNN_F16;
        auto* const upload_map = f16 ? upload_f16 : upload_f32;
        DevBuf dm[4], dr, dout, dflags;
        PyramidMaps pm;
        for (int l = 0; l < 4; ++l) {
            MRCNN_REQUIRE(maps[l] && heights[l] > 0 && widths[l] > 0, MRCNN_ERR_INVALID, "test_roi_align_nhwc_batch: level %d missing", l);
            const size_t per = (size_t)heights[l] * widths[l] * channels;
            upload_map(dm[l], maps[l], per * batch, 0);
            pm.data[l] = dm[l].p; pm.H[l] = heights[l]; pm.W[l] = widths[l]; pm.sB[l] = (long)per; pm.mul[l] = level_mul[l];
        }
        const long rois_sB = (long)n_rois * roi_stride, row = (long)pool * pool * channels, out_sB = (long)n_rois * row;
        upload_f32(dr, rois, (size_t)batch * rois_sB);
        const size_t n_out = (size_t)batch * out_sB;
        dout.alloc(n_out * (f16 ? 2 : 4));
        HIP_CHECK(hipMemset(dout.p, 0xff, n_out * (f16 ? 2 : 4)));      // an element the kernel skips comes back as NaN
        if (row_flags) {
            dflags.alloc((size_t)batch * n_rois * 4);
            HIP_CHECK(hipMemset(dflags.p, 0xff, (size_t)batch * n_rois * 4));
        }
        Stream st;
        roi_align_forward(st.s, pm, channels, 1, dr.as<float>(), rois_sB, roi_stride, n_rois, batch, pool, image_w, image_h, dout.p, out_sB, row, dtype,
                          row_flags ? dflags.as<int32_t>() : nullptr);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (f16) download_f16_as_f32(dout.p, n_out, out);
        else HIP_CHECK(hipMemcpy(out, dout.p, n_out * 4, hipMemcpyDeviceToHost));
        if (row_flags) HIP_CHECK(hipMemcpy(row_flags, dflags.p, (size_t)batch * n_rois * 4, hipMemcpyDeviceToHost));
    });
}

// proposal_forward on a BATCH of caller (host) images in ONE launch sequence, bound and strided the way MaskRCNNModel::predict does it: per-image
// state / hist / count words, blockIdx.y / z = image, nms_col_splits(W, B) — what the layer API (B = 1, every batch stride 0) never reaches
// (tests/test_gpu_boxes.py).  rois is IN/OUT: the caller's buffer is staged in first, as ProposalLayer.evaluate does.
extern "C" int mrcnn_test_proposals_batch(const float* probs, const float* deltas, const float* anchors, int batch, int n_anchors, const float std4[4],
                                          int pre_nms, int max_proposals, float nms_thr, float* rois, int64_t row_stride, int32_t* keep_count)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(probs && deltas && anchors && std4 && rois, MRCNN_ERR_INVALID, "test_proposals_batch: null argument");
        MRCNN_REQUIRE(batch >= 1 && n_anchors >= 1 && pre_nms >= 1 && max_proposals >= 1 && row_stride >= 4, MRCNN_ERR_INVALID,
                      "bad test_proposals_batch argument");
        MRCNN_REQUIRE(n_anchors < (1 << 24) / 4, MRCNN_ERR_UNSUPPORTED, "test_proposals_batch: region count exceeds the reference's float-index range");
        const int A = n_anchors, K = A < pre_nms ? A : pre_nms;
        const long rois_sB = (long)max_proposals * row_stride;
        DevBuf dp, dd, da, dr, ws_buf;
        upload_f32(dp, probs, (size_t)batch * A * 2);
        upload_f32(dd, deltas, (size_t)batch * A * 4);
        upload_f32(da, anchors, (size_t)A * 4);
        upload_f32(dr, rois, (size_t)batch * rois_sB);
        ProposalWorkspace ws;
        ws_buf.alloc(ProposalWorkspace::bytes(batch, A, K, max_proposals));
        ws.bind(ws_buf.p, batch, A, K, max_proposals);
        Stream st;
        Drain drain{st.s};
        proposal_forward(st.s, ws, dp.as<float>(), (long)A * 2, dd.as<float>(), (long)A * 4, da.as<float>(), std4, nms_thr, dr.as<float>(), rois_sB,
                         row_stride);
        HIP_CHECK(hipStreamSynchronize(st.s));
        HIP_CHECK(hipMemcpy(rois, dr.p, (size_t)batch * rois_sB * 4, hipMemcpyDeviceToHost));
        if (keep_count) HIP_CHECK(hipMemcpy(keep_count, ws.keep_count, (size_t)batch * 4, hipMemcpyDeviceToHost));
    });
}

// detection_forward on a batch of caller (host) images in one launch sequence, as MaskRCNNModel::predict calls it.  out is IN/OUT.
extern "C" int mrcnn_test_detections_batch(const float* rois, const float* cls6, int batch, int n, const float std4[4], int max_det, float score_thr,
                                           float nms_thr, float* out, int64_t row_stride)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(rois && cls6 && std4 && out, MRCNN_ERR_INVALID, "test_detections_batch: null argument");
        MRCNN_REQUIRE(batch >= 1 && n >= 1 && max_det >= 1 && row_stride >= 6, MRCNN_ERR_INVALID, "bad test_detections_batch argument");
        const long out_sB = (long)max_det * row_stride;
        DevBuf dr, dc, dout, ws_buf;
        upload_f32(dr, rois, (size_t)batch * n * 4);
        upload_f32(dc, cls6, (size_t)batch * n * 6);
        upload_f32(dout, out, (size_t)batch * out_sB);
        DetectionWorkspace ws;
        ws_buf.alloc(DetectionWorkspace::bytes(batch, n, max_det));
        ws.bind(ws_buf.p, batch, n, max_det);
        Stream st;
        Drain drain{st.s};
        detection_forward(st.s, ws, dr.as<float>(), (long)n * 4, 4, dc.as<float>(), (long)n * 6, std4, score_thr, nms_thr, 0, dout.as<float>(), out_sB,
                          row_stride);
        HIP_CHECK(hipStreamSynchronize(st.s));
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t)batch * out_sB * 4, hipMemcpyDeviceToHost));
    });
}

// The mask head's row selection on a batch of caller (host) images in one launch sequence, as MaskRCNNModel::predict binds it (engine.hip: the
// compaction over the row flags, then the fused or the unfused tail) or, with pooled rows and form 2, as TimeDistributedMaskLayer.evaluate does (api.hip:
// the predicate over d feature rows, the select over det_rows detections) — the workspace's rows per image are det_rows for both.  out is IN/OUT and is
// not zeroed here (tests/test_gpu_mask_select.py).
extern "C" int mrcnn_test_mask_select_batch(const mrcnn_test_mask_select* sel)
{
    return guarded([&] {
        require_gpu();
        MRCNN_REQUIRE(sel, MRCNN_ERR_INVALID, "test_mask_select_batch: null descriptor");
        const mrcnn_test_mask_select& q = *sel;
        const int form = q.form, B = q.batch, D = q.d, R = q.det_rows, HW = q.hw, C = q.c, nc = q.nc, parts = q.parts;
        MRCNN_REQUIRE(form >= 0 && form <= 2, MRCNN_ERR_INVALID, "test_mask_select_batch: form %d outside 0..2", form);
        MRCNN_REQUIRE(q.dtype == MRCNN_F32 || q.dtype == MRCNN_F16, MRCNN_ERR_INVALID, "test_mask_select_batch: dtype %d", q.dtype);
        MRCNN_REQUIRE(B >= 1 && D >= 1 && HW >= 1 && nc >= 1, MRCNN_ERR_INVALID, "test_mask_select_batch: batch %d, d %d, hw %d, nc %d: none may be below 1", B, D, HW, nc);
        MRCNN_REQUIRE(R >= D, MRCNN_ERR_INVALID, "test_mask_select_batch: det_rows %d < d %d", R, D);
        MRCNN_REQUIRE(q.det && q.out, MRCNN_ERR_INVALID, "test_mask_select_batch: null det or out");
        MRCNN_REQUIRE((q.flags != nullptr) != (q.pooled != nullptr), MRCNN_ERR_INVALID, "test_mask_select_batch: exactly one of flags and pooled gives the predicate");
        MRCNN_REQUIRE(q.det_stride >= 6 && q.out_stride >= HW, MRCNN_ERR_INVALID, "test_mask_select_batch: det_stride %ld < 6 or out_stride %ld < hw %d",
                      (long)q.det_stride, (long)q.out_stride, HW);
        if (q.pooled)
            MRCNN_REQUIRE(q.row_len >= 1 && q.row_stride >= q.row_len && q.pooled_batch_stride >= (int64_t)D * q.row_stride, MRCNN_ERR_INVALID,
                          "test_mask_select_batch: row_len %ld, row_stride %ld, pooled_batch_stride %ld", (long)q.row_len, (long)q.row_stride, (long)q.pooled_batch_stride);
        if (form == 0) {
            MRCNN_REQUIRE(q.feat && q.w && q.bias, MRCNN_ERR_INVALID, "test_mask_select_batch: form 0 needs feat, w and bias");
            MRCNN_REQUIRE(C >= 4 && C % 4 == 0, MRCNN_ERR_SHAPE, "test_mask_select_batch: c %d is not a positive multiple of 4", C);
        } else if (form == 1) {
            MRCNN_REQUIRE(q.partial && q.bias, MRCNN_ERR_INVALID, "test_mask_select_batch: form 1 needs partial and bias");
            MRCNN_REQUIRE(parts >= 1, MRCNN_ERR_INVALID, "test_mask_select_batch: parts %d < 1", parts);
        } else {
            MRCNN_REQUIRE(q.masks, MRCNN_ERR_INVALID, "test_mask_select_batch: form 2 needs masks");
        }
        const bool f16 = q.dtype == MRCNN_F16;
        const long det_sB = (long)R * q.det_stride, out_sB = (long)R * q.out_stride;

        // the workspace: R rows per image, -1 wherever no launch writes
        Carver carve;
        const auto s_flags = carve.take<int32_t>((size_t)B * R), s_map = carve.take<int32_t>((size_t)B * R), s_cid = carve.take<int32_t>((size_t)B * R);
        const auto s_kept = carve.take<int32_t>((size_t)B);
        carve.alloc();
        HIP_CHECK(hipMemset(carve.buf.p, 0xff, carve.size));
        MaskSelectWorkspace ws;
        ws.flags = carve[s_flags]; ws.mapping = carve[s_map]; ws.sel_cid = carve[s_cid]; ws.kept = carve[s_kept]; ws.ld = R;
        auto rows_to_host = [&](int32_t* dst, const int32_t* dev, int n) {
            HIP_CHECK(hipMemcpy2D(dst, (size_t)n * 4, dev, (size_t)R * 4, (size_t)n * 4, (size_t)B, hipMemcpyDeviceToHost));
        };

        DevBuf dpool, ddet, dout, dfeat, dw, dbias, dpart, dmasks;
        if (q.flags) HIP_CHECK(hipMemcpy2D(ws.flags, (size_t)R * 4, q.flags, (size_t)D * 4, (size_t)D * 4, (size_t)B, hipMemcpyHostToDevice));
        else (f16 ? upload_f16 : upload_f32)(dpool, q.pooled, (size_t)B * q.pooled_batch_stride, 0);
        upload_f32(ddet, q.det, (size_t)B * det_sB);
        upload_f32(dout, q.out, (size_t)B * out_sB);
        if (form == 0) {
            (f16 ? upload_f16 : upload_f32)(dfeat, q.feat, (size_t)B * D * HW * C, 0);
            upload_f32(dw, q.w, (size_t)nc * C);
        }
        if (form != 2) upload_f32(dbias, q.bias, (size_t)nc);
        if (form == 1) {                               // k_mask_select_partials strides the images by the rows it pads: R rows each, zero behind the first D
            const size_t row = (size_t)HW * parts;
            dpart.alloc((size_t)B * R * row * 4);
            HIP_CHECK(hipMemset(dpart.p, 0, (size_t)B * R * row * 4));
            HIP_CHECK(hipMemcpy2D(dpart.p, (size_t)R * row * 4, q.partial, (size_t)D * row * 4, (size_t)D * row * 4, (size_t)B, hipMemcpyHostToDevice));
        }
        if (form == 2) upload_f32(dmasks, q.masks, (size_t)B * D * nc * HW);

        Stream st;
        Drain drain{st.s};
        mask_valid_rows_forward(st.s, q.pooled ? dpool.p : nullptr, (long)q.pooled_batch_stride, (long)q.row_stride, (long)q.row_len, D, B, ws, q.dtype);
        if (form == 1 || q.sel_cid) mask_select_classes(st.s, ddet.as<float>(), det_sB, (long)q.det_stride, R, B, nc, ws, ws.sel_cid);
        if (form == 0)
            mask_select_forward(st.s, dfeat.p, (long)D * HW * C, HW, C, dw.as<float>(), dbias.as<float>(), nc, ddet.as<float>(), det_sB, (long)q.det_stride, R, B, ws,
                                dout.as<float>(), out_sB, (long)q.out_stride, q.dtype);
        else if (form == 1)
            mask_select_from_partials(st.s, dpart.as<float>(), parts, HW, dbias.as<float>(), nc, ddet.as<float>(), det_sB, (long)q.det_stride, R, B, ws,
                                      dout.as<float>(), out_sB, (long)q.out_stride);
        else
            mask_select_from_full_forward(st.s, dmasks.as<float>(), (long)D * nc * HW, HW, nc, ddet.as<float>(), det_sB, (long)q.det_stride, R, B, ws,
                                          dout.as<float>(), out_sB, (long)q.out_stride);
        HIP_CHECK(hipStreamSynchronize(st.s));
        HIP_CHECK(hipMemcpy(q.out, dout.p, (size_t)B * out_sB * 4, hipMemcpyDeviceToHost));
        if (q.row_flags) rows_to_host(q.row_flags, ws.flags, D);
        if (q.mapping) rows_to_host(q.mapping, ws.mapping, D);
        if (q.sel_cid) rows_to_host(q.sel_cid, ws.sel_cid, R);
        if (q.kept) HIP_CHECK(hipMemcpy(q.kept, ws.kept, (size_t)B * 4, hipMemcpyDeviceToHost));
    });
}

extern "C" int mrcnn_model_conv_profile_enable(mrcnn_model* model, int on)
{
    return guarded([&] {
        MRCNN_REQUIRE(model, MRCNN_ERR_INVALID, "null model");
        ConvProfile& cp = model->m.conv_profile;
        if (on) {
            cp.reset();                                  // a new measurement window
        } else if (cp.active) {
            HIP_CHECK(hipStreamSynchronize(model->m.stream));
            cp.collect();                                // keep the totals readable after the window closes
        }
        cp.active = on != 0;
    });
}
extern "C" int mrcnn_model_conv_profile_get(mrcnn_model* model, int tile, int64_t* launches, double* total_ms, double* total_flops)
{
    return guarded([&] {
        MRCNN_REQUIRE(model && launches && total_ms && total_flops && tile >= 0 && tile < TILE_CLASSES, MRCNN_ERR_INVALID, "bad argument");
        HIP_CHECK(hipStreamSynchronize(model->m.stream));
        model->m.conv_profile.collect();
        const auto& sl = model->m.conv_profile.by_tile[tile];
        *launches = sl.launches; *total_ms = sl.ms; *total_flops = sl.flops;
    });
}

extern "C" int mrcnn_model_conv_profile_bytes(mrcnn_model* model, int tile, double* total_bytes)
{
    return guarded([&] {
        MRCNN_REQUIRE(model && total_bytes && tile >= 0 && tile < TILE_CLASSES, MRCNN_ERR_INVALID, "bad argument");
        HIP_CHECK(hipStreamSynchronize(model->m.stream));
        model->m.conv_profile.collect();
        *total_bytes = model->m.conv_profile.by_tile[tile].bytes;
    });
}

extern "C" int mrcnn_model_conv_profile_group(mrcnn_model* model, int group, int64_t* launches, double* total_ms, double* total_flops)
{
    return guarded([&] {
        MRCNN_REQUIRE(model && launches && total_ms && total_flops && (group == 0 || group == 1), MRCNN_ERR_INVALID, "bad argument");
        // (the totals are complete only once the pending launches' events have been read — as in _get)
        HIP_CHECK(hipStreamSynchronize(model->m.stream));
        model->m.conv_profile.collect();
        const auto& sl = model->m.conv_profile.by_group[group];
        *launches = sl.launches; *total_ms = sl.ms; *total_flops = sl.flops;
    });
}
extern "C" int mrcnn_model_conv_profile_shapes(mrcnn_model* model, mrcnn_conv_shape_stat* out, int capacity, int* count)
{
    return guarded([&] {
        MRCNN_REQUIRE(model && count && (out || capacity == 0) && capacity >= 0, MRCNN_ERR_INVALID, "bad argument");
        HIP_CHECK(hipStreamSynchronize(model->m.stream));
        model->m.conv_profile.collect();
        const auto& shapes = model->m.conv_profile.by_shape;
        *count = (int)shapes.size();
        int i = 0;
        for (const auto& kv : shapes) {
            if (i >= capacity) break;
            out[i++] = {kv.first.M, kv.first.N, kv.first.K, kv.first.tile, (int64_t)kv.second.launches, kv.second.ms, kv.second.flops, kv.second.bytes};
        }
    });
}

// The inverse mrcnn_rle_transform's device entry works from (transform_rule.h's xf_preimage), on the host: the closed form can be pinned
// against brute force without a GPU (tests/test_rle_transform_host.py).
extern "C" int mrcnn_test_xf_preimage(int64_t a, int64_t b, int64_t A, int64_t B, int64_t D, int64_t* lo, int64_t* hi)
{
    return guarded([&] {
        MRCNN_REQUIRE(lo && hi, MRCNN_ERR_INVALID, "test_xf_preimage: null output");
        MRCNN_REQUIRE(a <= b && a >= -32768 && b <= 32768, MRCNN_ERR_SHAPE, "test_xf_preimage: the source range [%lld, %lld) must be ordered and lie within +-32768",
                      (long long)a, (long long)b);
        MRCNN_REQUIRE(xf_axis_known(A, B, D), MRCNN_ERR_SHAPE, "test_xf_preimage: A, B, D = %lld, %lld, %lld: 1 <= |A|, D <= 2^31-1 and |B| <= 2^46 expected",
                      (long long)A, (long long)B, (long long)D);
        long long l, h;
        xf_preimage(XfAxis{(long long)A, (long long)B, (long long)D}, a, b, &l, &h);
        *lo = l; *hi = h;
    });
}
