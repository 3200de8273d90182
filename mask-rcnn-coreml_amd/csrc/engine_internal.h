// engine_internal.h — what the engine's own files (engine.hip, engine_weights.hip, engine_heads.hip, engine_plan.hip,
// engine_split.hip) share with each other and nobody else: the upload helpers, the packers, the one ConvDesc maker and the
// lay-out-twice idiom of the arenas.  The api_*.hip files and dist.hip see engine.h only.
#pragma once
#include "engine.h"

namespace mrcnn {

// ---- engine_weights.hip ---------------------------------------------------------------------------------------------
float half_to_float(uint16_t h);
void upload(DevBuf& d, const std::vector<float>& h);
// kernel [O][I][KH][KW] (Core ML layout) → [Npad][KH][KW][I], BatchNorm `bn` ("" = none) folded into scale / shift
PackedConv pack_conv_oihw(const MrcwFile& f, const std::string& conv, const std::string& bn, int mode);
PackedConv pack_conv1(const MrcwFile& f, int mode);
PackedConv pack_stacked_1x1(const MrcwFile& f, const std::vector<std::string>& names, int mode);
PackedConv pack_deconv2(const MrcwFile& f, const std::string& name, int mode);
void init_scaled_op(ScaledOp& op, const PackedConv* pc, int g_in, int g_out);      // allocates the copies = the base scale / shift

// ---- the one ConvDesc maker -----------------------------------------------------------------------------------------
// What a convolution reads or writes: an NHWC tensor (channel stride 1) with its three outer strides in elements.  A dense
// Tensor4 converts; the padded stem input, the sub-sampled P6 read and the deconvolution's interleaved output are views
// with other strides.
struct ConvView {
    void* p = nullptr;
    int H = 0, W = 0;
    long sB = 0, sH = 0, sW = 0;
};
inline ConvView dense_view(const void* p, int H, int W, int C)
{
    return {const_cast<void*>(p), H, W, (long)H * W * C, (long)W * C, (long)C};
}
inline ConvView view_of(const Tensor4& t) { return dense_view(t.p, t.H, t.W, t.C); }

// Which re-tiled copies of its filters a site hands to the dispatcher.  conv_forward reads a non-null pointer as permission to
// run that kernel, so this is a dispatch decision of the SITE: a pack may hold a copy its site does not pass.
enum : unsigned { RETILED_NONE = 0, RETILED_HALO = 1, RETILED_C3H = 2, RETILED_FRAG = 4, RETILED_STREAM = 8, RETILED_ALL = 15 };

// Everything a ConvDesc takes from its pack, its two views and (stride, pad, act); B stays 0 (set per call).  A site then adds
// only what is particular to it: algo_k / group, out_f32 / out2* / n_split, head_*, deconv2 / out_sH / out_sW / sel_*, res*.
inline ConvDesc make_conv_desc(const PackedConv& pc, const float* scale, const float* shift, const ConvView& in, const ConvView& out,
                               int stride, int pad, int act, unsigned retiled)
{
    ConvDesc d;
    d.dtype = pc.dtype; d.wdtype = pc.wdtype;
    d.in = in.p; d.H = in.H; d.W = in.W; d.Cin = pc.Cin;
    d.in_sB = in.sB; d.in_sH = in.sH; d.in_sW = in.sW;
    d.wgt = pc.wgt.p; d.KH = pc.KH; d.KW = pc.KW; d.stride = stride; d.padH = d.padW = pad;
    if (retiled & RETILED_HALO) d.wgt_halo = pc.wgt_halo.p;
    if (retiled & RETILED_C3H) d.wgt_c3h = pc.wgt_c3h.p;
    if (retiled & RETILED_FRAG) d.wgt_frag = pc.wgt_frag.p;
    if (retiled & RETILED_STREAM) d.wgt_stream = pc.wgt_stream.p;
    d.scale = scale; d.shift = shift;
    d.act = act;
    d.out = out.p; d.OH = out.H; d.OW = out.W; d.Cout = pc.Cout; d.Npad = pc.Npad;
    d.out_sB = out.sB; d.out_sP = out.sW;            // (rows of the image contiguous: out.sH is the deconvolution's business)
    return d;
}
inline void set_residual(ConvDesc& d, const ConvView& res, int res_shift)
{
    d.res = res.p; d.res_sB = res.sB; d.res_sH = res.sH; d.res_sW = res.sW; d.res_shift = res_shift;
}

// Dense NHWC conv helper of the heads (in: B×H×W×Cin, out: B×OH×OW×Cout).
void run_conv_dense(hipStream_t s, const PackedConv& pc, const void* in, int B, int H, int W, void* out, int stride,
                    int pad, int act, const void* res = nullptr, int out_f32 = 0, const ScaledOp* sop = nullptr);

// ---- arenas ---------------------------------------------------------------------------------------------------------
// Lay out twice, allocate in between: the first run of `lay_out(ar, real = false)` only sizes the arena (null base: every
// pointer it hands out is null), the second binds the real pointers.  Both runs must ask for the same things in the same order.
template <class F>
void lay_out_twice(DevBuf& arena, F&& lay_out)
{
    Arena ar;
    lay_out(ar, false);
    arena.alloc(ar.off);
    ar.base = arena.as<char>();
    ar.off = 0;
    lay_out(ar, true);
}

}  // namespace mrcnn
