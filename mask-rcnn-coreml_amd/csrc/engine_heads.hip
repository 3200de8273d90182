// engine_heads.hip — the two heads behind the ROIAlign passes (Classifier.mlmodel, Mask.mlmodel), as parts of the fused model and
// as the stand-alone models of the TimeDistributed*Layer plugins.
#include "engine_internal.h"

namespace mrcnn {

// Dense NHWC conv helper (in: B×H×W×Cin, out: B×OH×OW×Cout).
void run_conv_dense(hipStream_t s, const PackedConv& pc, const void* in, int B, int H, int W, void* out, int stride,
                    int pad, int act, const void* res, int out_f32, const ScaledOp* sop)
{
    const int OH = (H + 2 * pad - pc.KH) / stride + 1, OW = (W + 2 * pad - pc.KW) / stride + 1;
    const ConvView vo = dense_view(out, OH, OW, pc.Cout);
    // RETILED_HALO only, deliberately: wgt_c3h / wgt_frag stay null here, which is why the mask head's 3x3 layers do not take the fp16
    // halo-tile kernel.  Passing them is a dispatch change with its own measurement, not part of describing the layer.
    ConvDesc d = make_conv_desc(pc, (sop ? sop->scale : pc.scale).as<float>(), (sop ? sop->shift : pc.shift).as<float>(),
                                dense_view(in, H, W, pc.Cin), vo, stride, pad, act, RETILED_HALO);
    d.B = B; d.out_f32 = out_f32;
    if (res) set_residual(d, dense_view(res, OH, OW, pc.Cout), 0);
    conv_forward(s, d);
}

// ------------------------------------------------------------------------------------------------
// Classifier head
// ------------------------------------------------------------------------------------------------
void ClassifierHead::load(const MrcwFile& f, int capacity_rows, int dtype_)
{
    nc = (int)f.get_int("num_classes");
    cap = capacity_rows;
    mode = dtype_;
    dtype = mode_act(mode);
    const MrcwTensor& k1 = f.tensor("mrcnn_class_conv1/kernel");
    MRCNN_REQUIRE(k1.dims.size() == 4, MRCNN_ERR_IO, "mrcnn_class_conv1/kernel must be 4-D");
    C = k1.dims[1]; pool = k1.dims[2];
    fc1 = pack_conv_oihw(f, "mrcnn_class_conv1", "mrcnn_class_bn1", mode);    // [1024][7][7][256] == rows of the NHWC pooled vector
    fc1.Cin = fc1.Cin * fc1.KH * fc1.KW; fc1.KH = fc1.KW = 1;           // as an inner product over K = 12544
    fc2 = pack_conv_oihw(f, "mrcnn_class_conv2", "mrcnn_class_bn2", mode);
    fc3 = pack_stacked_1x1(f, {"mrcnn_class_logits", "mrcnn_bbox_fc"}, mode);
    MRCNN_REQUIRE(fc3.Cout == 5 * nc, MRCNN_ERR_IO, "classifier output size %d != 5*num_classes", fc3.Cout);
    lay_out_twice(arena, [&](Arena& ar, bool) {
        h1 = ar.alloc_e((size_t)cap * fc1.Cout, dtype);
        h2 = ar.alloc_e((size_t)cap * fc2.Cout, dtype);
        lb = ar.alloc_f((size_t)cap * fc3.Cout);
        probs = ar.alloc_f((size_t)cap * nc);
        bbox = ar.alloc_f((size_t)cap * nc * 4);
        cls6 = ar.alloc_f((size_t)cap * 6);
        stage_in = ar.alloc_e((size_t)cap * pool * pool * C, dtype);
    });
    init_scaled_op(sop[0], &fc1, -1, -1);
    init_scaled_op(sop[1], &fc2, -1, -1);
    init_scaled_op(sop[2], &fc3, -1, -1);
}

void ClassifierHead::forward(hipStream_t s, const void* pooled_nhwc, int n, float* cls6_out, long cls6_stride)
{
    MRCNN_REQUIRE(n <= cap, MRCNN_ERR_SHAPE, "classifier head: %d rows exceed capacity %d", n, cap);
    if (n <= 0) return;
    // rows are "pixels" of a 1×n image
    run_conv_dense(s, fc1, pooled_nhwc, 1, 1, n, h1, 1, 0, ACT_RELU, nullptr, 0, &sop[0]);
    if (observe) observe(s, grp[1], h1, (size_t)n * fc1.Cout);
    run_conv_dense(s, fc2, h1, 1, 1, n, h2, 1, 0, ACT_RELU, nullptr, 0, &sop[1]);
    if (observe) observe(s, grp[2], h2, (size_t)n * fc2.Cout);
    run_conv_dense(s, fc3, h2, 1, 1, n, lb, 1, 0, ACT_NONE, nullptr, 1, &sop[2]);
    TraceRange tr("TimeDistributedClassifierLayer-ProcessOutput");
    softmax_rows_forward(s, lb, fc3.Cout, nc, n, probs);
    copy_columns_forward(s, lb, fc3.Cout, nc, 4 * nc, n, bbox);
    if (cls6_out) classifier_postprocess_forward(s, probs, bbox, nc, n, cls6_out, cls6_stride);
}

// ------------------------------------------------------------------------------------------------
// Mask head
// ------------------------------------------------------------------------------------------------
void MaskHead::load(const MrcwFile& f, int capacity_rows, int dtype_)
{
    nc = (int)f.get_int("num_classes");
    cap = capacity_rows;
    mode = dtype_;
    dtype = mode_act(mode);
    for (int i = 0; i < 4; ++i)
        conv[i] = pack_conv_oihw(f, "mrcnn_mask_conv" + std::to_string(i + 1), "mrcnn_mask_bn" + std::to_string(i + 1), mode);
    C = conv[0].Cin;
    deconv = pack_deconv2(f, "mrcnn_mask_deconv", mode);
    final_full = pack_conv_oihw(f, "mrcnn_mask", "", mode);
    upload(final_w, f.floats("mrcnn_mask/kernel"));
    upload(final_b, f.floats("mrcnn_mask/bias"));
    const size_t hw = (size_t)pool * pool;
    lay_out_twice(arena, [&](Arena& ar, bool) {
        t0 = ar.alloc_e((size_t)cap * hw * C, dtype);
        t1 = ar.alloc_e((size_t)cap * hw * C, dtype);
        feat = ar.alloc_e((size_t)cap * hw * 4 * deconv.Cout, dtype);
        full = ar.alloc_f((size_t)cap * hw * 4 * nc);
        stage_in = ar.alloc_e((size_t)cap * hw * C, dtype);
    });
    for (int i = 0; i < 4; ++i) init_scaled_op(sop[i], &conv[i], -1, -1);
    init_scaled_op(sop[4], &deconv, -1, -1);
}

void MaskHead::forward_features(hipStream_t s, const void* pooled_nhwc, int n, const int32_t* sel_cid, float* sel_partial)
{
    MRCNN_REQUIRE(n <= cap, MRCNN_ERR_SHAPE, "mask head: %d rows exceed capacity %d", n, cap);
    if (n <= 0) return;
    const size_t te = (size_t)n * pool * pool * C;
    run_conv_dense(s, conv[0], pooled_nhwc, n, pool, pool, t0, 1, 1, ACT_RELU, nullptr, 0, &sop[0]);
    if (observe) observe(s, grp[1], t0, te);
    run_conv_dense(s, conv[1], t0, n, pool, pool, t1, 1, 1, ACT_RELU, nullptr, 0, &sop[1]);
    if (observe) observe(s, grp[2], t1, te);
    run_conv_dense(s, conv[2], t1, n, pool, pool, t0, 1, 1, ACT_RELU, nullptr, 0, &sop[2]);
    if (observe) observe(s, grp[3], t0, te);
    run_conv_dense(s, conv[3], t0, n, pool, pool, t1, 1, 1, ACT_RELU, nullptr, 0, &sop[3]);
    if (observe) observe(s, grp[4], t1, te);
    // the deconvolution as a GEMM over the pool x pool input pixels: output pixel (2oh+dy, 2ow+dx) of the 2pool x 2pool image, i.e. the
    // view of feat with one row of the OUTPUT as sH
    const int Co = deconv.Cout;
    const ConvView vo = {feat, pool, pool, (long)4 * pool * pool * Co, (long)2 * pool * Co, (long)Co};
    ConvDesc d = make_conv_desc(deconv, sop[4].scale.as<float>(), sop[4].shift.as<float>(), dense_view(t1, pool, pool, deconv.Cin), vo, 1, 0,
                                ACT_RELU, RETILED_NONE);
    d.B = n;
    d.deconv2 = 1; d.out_sH = vo.sH; d.out_sW = vo.sW;
    if (sel_partial) { d.sel_w = final_w.as<float>(); d.sel_cid = sel_cid; d.sel_partial = sel_partial; }   // feat is not written
    conv_forward(s, d);
}

void MaskHead::forward_full(hipStream_t s, int n)
{
    if (n <= 0) return;
    const int P2 = 2 * pool;
    ConvDesc d = make_conv_desc(final_full, final_full.scale.as<float>(), final_full.shift.as<float>(), dense_view(feat, P2, P2, final_full.Cin),
                                dense_view(full, P2, P2, nc), 1, 0, ACT_SIGMOID, RETILED_NONE);
    d.B = n; d.out_f32 = 1;
    d.Cout = nc;                 // (`full` holds nc columns per pixel: the store is bounded by the head's class count, whatever the artefact's O)
    conv_forward(s, d);
}

}  // namespace mrcnn
