// engine_split.hip — the scale-aware split (engine.h: SplitGroup): the groups and the per-op scale / shift copies that carry their
// exponents, the one kernel that observes a tensor during a calibration pass, calibration and range recovery.
#include "engine_internal.h"

#include <math.h>
#include <string.h>

namespace mrcnn {

// ------------------------------------------------------------------------------------------------
// scale-aware split (engine.h: SplitGroup)
// ------------------------------------------------------------------------------------------------
int Model::new_split_group(const std::string& name, bool fixed)
{
    SplitGroup g;
    g.name = name; g.fixed = fixed;
    sgroups.push_back(g);
    return (int)sgroups.size() - 1;
}

ScaledOp* Model::new_scaled_op(const PackedConv* pc, int g_in, int g_out)
{
    sops.emplace_back(new ScaledOp);
    init_scaled_op(*sops.back(), pc, g_in, g_out);
    return sops.back().get();
}

// max |x| of a tensor (phase 1) / how many of its non-zero elements the three-part split cannot carry exactly (phase 2):
// slot = [uint32 bits of the maximum | pad | small | inexact | counted] (32 B per group)
__global__ __launch_bounds__(256) void k_split_observe(const float* __restrict__ x, size_t n, int phase, float small_thr, unsigned* __restrict__ slot)
{
    const size_t stride = (size_t)gridDim.x * 256;
    float mx = 0.f;
    unsigned long long small = 0, inexact = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float a = fabsf(x[i]);
        if (phase == 1) mx = fmaxf(mx, a);
        else if (a != 0.f) { small += a < small_thr; inexact += a < 0.5f; }
    }
    __shared__ float s_mx[256];
    __shared__ unsigned long long s_a[256], s_b[256];
    s_mx[threadIdx.x] = mx; s_a[threadIdx.x] = small; s_b[threadIdx.x] = inexact;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + w]);
            s_a[threadIdx.x] += s_a[threadIdx.x + w];
            s_b[threadIdx.x] += s_b[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (phase == 1) atomicMax(slot, __float_as_uint(s_mx[0]));        // non-negative floats order like their bit patterns (NaN / inf sort above everything: reported)
        else {
            unsigned long long* c = reinterpret_cast<unsigned long long*>(slot + 2);
            atomicAdd(c, s_a[0]);
            atomicAdd(c + 1, s_b[0]);
            if (blockIdx.x == 0) atomicAdd(c + 2, (unsigned long long)n);
        }
    }
}

void Model::observe_split(hipStream_t s, int group, const void* x, size_t n)
{
    if (!calib_phase || group < 0 || n == 0 || dtype != MRCNN_F32) return;
    const SplitGroup& g = sgroups[(size_t)group];
    if (g.fixed) return;
    // phase 2 sees the stored (scaled) tensor: "small" = below 2^-8 of the group's maximum, "inexact" = below 0.5
    const float small_thr = ldexpf(g.absmax, g.exp - 8);
    const int grid = (int)((n + 256 * 16 - 1) / (256 * 16) < 2048 ? (n + 256 * 16 - 1) / (256 * 16) : 2048);
    hipLaunchKernelGGL(k_split_observe, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, static_cast<const float*>(x), n, calib_phase, small_thr,
                       calib_buf.as<unsigned>() + (size_t)group * 8);
    HIP_CHECK(hipGetLastError());
}

void Model::apply_split_exponents()
{
    HIP_CHECK(hipStreamSynchronize(stream));
    drop_graphs();                                   // the fused heads' multiplier and the samplers' are launch arguments
    auto ex = [&](int g) { return g >= 0 ? sgroups[(size_t)g].exp : 0; };
    auto refresh = [&](ScaledOp& op) {
        const int ds = ex(op.g_out) - ex(op.g_in), eo = ex(op.g_out);
        std::vector<float> sc(op.pc->h_scale), sh(op.pc->h_shift);
        for (auto& v : sc) v = ldexpf(v, ds);        // exact: a power of two (a folded BatchNorm scale is nowhere near the fp32 range limits)
        for (auto& v : sh) v = ldexpf(v, eo);
        HIP_CHECK(hipMemcpy(op.scale.p, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(op.shift.p, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    };
    for (auto& op : sops) refresh(*op);
    for (auto& op : cls_head.sop) refresh(op);
    for (auto& op : mask_head.sop) refresh(op);
}

// Restores the exponent vector it saw when it was made, and re-applies it, on every way out of its scope — unless dismissed.
// (Leaving by an exception, a failure of the restore itself is dropped: the caller sees the exception that caused it.)
namespace {
struct ExponentGuard {
    Model& m;
    std::vector<int> saved;
    bool armed = true;
    explicit ExponentGuard(Model& model) : m(model) { for (auto& g : m.sgroups) saved.push_back(g.exp); }
    void dismiss() { armed = false; }
    void restore_now()
    {
        armed = false;
        for (size_t g = 0; g < saved.size(); ++g) m.sgroups[g].exp = saved[g];
        m.apply_split_exponents();
    }
    ~ExponentGuard() { if (armed) try { restore_now(); } catch (...) {} }
};
}  // namespace

int Model::split_exponent_for(float absmax)
{
    if (!(absmax > 0.f)) return 0;
    int k = 0;
    (void)frexpf(absmax, &k);                      // absmax = m * 2^k, 0.5 <= m < 1
    const int e = 12 - k;
    return e < -24 ? -24 : (e > 48 ? 48 : e);
}

void Model::measure_split_groups(const uint8_t* rgb, int batch, int h, int w, int memspace, bool fit, bool resident)
{
    const size_t G = sgroups.size();
    std::vector<unsigned> raw(G * 8);
    // true magnitudes.  Every exponent 0 — or, when an activation of THIS model leaves the fp16 range there (the watchdog fails the
    // pass: its maxima would be garbage), one uniform negative exponent that keeps it inside
    int base = 0;
    for (;;) {
        for (auto& g : sgroups) g.exp = g.fixed ? 0 : base;
        apply_split_exponents();
        HIP_CHECK(hipMemset(calib_buf.p, 0, G * 32));
        calib_phase = 1;
        bool tripped = false;
        try {
            predict(rgb, batch, h, w, memspace, nullptr, nullptr, true, fit, resident);
        } catch (const Error& e) {
            calib_phase = 0;
            if (e.code != MRCNN_ERR_UNSUPPORTED || base <= -36) throw;
            tripped = true;
        } catch (...) {
            calib_phase = 0;
            throw;
        }
        calib_phase = 0;
        if (!tripped) break;
        base -= 6;
    }
    HIP_CHECK(hipMemcpy(raw.data(), calib_buf.p, G * 32, hipMemcpyDeviceToHost));
    for (size_t g = 0; g < G; ++g) {
        float mx;
        memcpy(&mx, &raw[g * 8], 4);
        mx = ldexpf(mx, -sgroups[g].exp);               // stored = 2^e * value
        sgroups[g].absmax = mx;
        MRCNN_REQUIRE(mx == mx && mx < 3.0e38f, MRCNN_ERR_UNSUPPORTED, "%s: tensor group '%s' holds inf / NaN on this batch (an fp32 engine would produce them too)",
                      resident ? "range recovery of a predict (the batch was measured where it sits, after an activation left the fp16 range)" : "calibrate_split",
                      sgroups[g].name.c_str());
    }
}

void Model::calibrate_split(const uint8_t* rgb, int batch, int h, int w, int memspace, bool apply)
{
    MRCNN_REQUIRE(kind == MRCNN_MODEL_MASKRCNN, MRCNN_ERR_INVALID, "calibrate_split called on a non-MaskRCNN model");
    MRCNN_REQUIRE(mode == MRCNN_F32S || mode == MRCNN_F32X3, MRCNN_ERR_UNSUPPORTED,
                  "calibrate_split: only the split modes (MRCNN_F32S, MRCNN_F32X3) carry activations through fp16 parts; this model is scale-invariant as it is");
    MRCNN_REQUIRE(batch >= 1 && batch <= max_batch, MRCNN_ERR_SHAPE, "batch %d outside 1..%d", batch, max_batch);
    const size_t G = sgroups.size();
    std::vector<unsigned> raw(G * 8);
    ExponentGuard keep(*this);
    // ---- phase 1: true magnitudes ----
    measure_split_groups(rgb, batch, h, w, memspace, false, false);
    // ---- exponents: max |a| * 2^e in [2^11, 2^12) — 16x head room below the fp16 range, 0.5 = 2^-13 of the maximum exact ----
    std::vector<int> chosen(G, 0);
    for (size_t g = 0; g < G; ++g)
        if (!sgroups[g].fixed) chosen[g] = split_exponent_for(sgroups[g].absmax);
    // ---- phase 2: with the chosen exponents — verifies them (range watchdog) and counts what a split still cannot carry.
    //      (The images are resident from phase 1: no second copy, and a device-side caller's buffer is read once.) ----
    for (size_t g = 0; g < G; ++g) sgroups[g].exp = chosen[g];
    apply_split_exponents();
    HIP_CHECK(hipMemset(calib_buf.p, 0, G * 32));
    calib_phase = 2;
    try {
        predict(rgb, batch, h, w, memspace, nullptr, nullptr, true, false, true);
    } catch (...) {
        calib_phase = 0;
        throw;
    }
    calib_phase = 0;
    HIP_CHECK(hipMemcpy(raw.data(), calib_buf.p, G * 32, hipMemcpyDeviceToHost));
    for (size_t g = 0; g < G; ++g) {
        unsigned long long c[3];
        memcpy(c, &raw[g * 8 + 2], 24);
        sgroups[g].small = (long long)c[0]; sgroups[g].inexact = (long long)c[1]; sgroups[g].counted = (long long)c[2];
    }
    if (!apply) keep.restore_now();
    else { split_calibrated = true; keep.dismiss(); }
}

bool Model::recover_range(int batch, int h, int w, bool fit)
{
    if (!(mode == MRCNN_F32S || mode == MRCNN_F32X3) || kind != MRCNN_MODEL_MASKRCNN) return false;
    const size_t G = sgroups.size();
    ExponentGuard keep(*this);
    const std::vector<int>& before = keep.saved;
    try {
        measure_split_groups(nullptr, batch, h, w, MRCNN_DEVICE, fit, true);
    } catch (const Error& e) {
        // (the caller asked for a predict, not for a calibration: say what happened in ITS terms — ADVICE r5)
        fail(e.code, "predict: an activation left the calibrated fp16 range and the batch could not be measured for a range recovery (%s); the split "
             "exponents are unchanged, the results of this call are not valid", e.msg.c_str());
    }
    // never raise an exponent: what earlier batches needed still fits
    for (size_t g = 0; g < G; ++g) {
        if (sgroups[g].fixed) { sgroups[g].exp = 0; continue; }
        const int need = split_exponent_for(sgroups[g].absmax);
        sgroups[g].exp = need < before[g] ? need : before[g];
    }
    keep.dismiss();
    apply_split_exponents();
    return true;
}

}  // namespace mrcnn
