// engine_plan.hip — Model::load and, for the MaskRCNN model, the plan builder: configuration, sub-artefacts, trunk weights, and the
// static activation plan (arena layout, split groups, taps and the ops Model::enqueue_pipeline replays).
#include "engine_internal.h"

#include <math.h>
#include <string.h>

#include <fstream>

namespace mrcnn {

static void read_std(const MrcwFile& f, const std::string& prefix, float out[4])
{
    const float dflt[4] = {0.1f, 0.1f, 0.2f, 0.2f};
    const int64_t cnt = f.get_int(prefix + "bboxStdDev_count", 0);
    for (int i = 0; i < 4; ++i) out[i] = dflt[i];
    if (cnt == 4)
        for (int i = 0; i < 4; ++i) out[i] = (float)f.get_double(prefix + "bboxStdDev_" + std::to_string(i), dflt[i]);
}

void Model::load(int kind_, const std::string& path, int max_batch_, int dtype_)
{
    require_gpu();
    kind = kind_;
    max_batch = max_batch_ > 0 ? max_batch_ : 1;
    file.load(path);
    mode = dtype_;
    if (dtype_ == MRCNN_DEFAULT) {
        // the mode the artefact is prepared for (include/maskrcnn_hip.h): stored split exponents -> the three-part split, else exact fp32
        bool stored = false;
        if (kind == MRCNN_MODEL_MASKRCNN)
            for (auto& kv : file.ints) stored = stored || kv.first.compare(0, 10, "split_exp.") == 0;
        mode = stored ? MRCNN_F32X3 : MRCNN_F32;
        mode_defaulted = true;
    }
    dtype = mode_act(mode);
    const char* want = kind == MRCNN_MODEL_MASKRCNN ? "MaskRCNN" : kind == MRCNN_MODEL_CLASSIFIER ? "Classifier" : "Mask";
    MRCNN_REQUIRE(file.get_string("kind") == want, MRCNN_ERR_IO, "'%s' holds a %s model, expected %s", path.c_str(),
                  file.get_string("kind").c_str(), want);
    if (const char* cm = knob_env("MRCNN_CU_MASK_PROBE")) {
        fprintf(stderr, "libmaskrcnn_hip: MRCNN_CU_MASK_PROBE — this handle's stream runs on a subset of the CUs (measurement only)\n");
        // measurement only (tools/dual_stream_probe.py): the handle's stream on a subset of the CUs — 8 hexadecimal words, "w0,w1,...,w7"
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int n = 0;
        for (const char* p = cm; *p && n < 8; ++n) { words[n] = (uint32_t)strtoul(p, nullptr, 16); p = strchr(p, ','); if (!p) { ++n; break; } ++p; }
        HIP_CHECK(hipExtStreamCreateWithCUMask(&stream, 8, words));
    } else
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
    if (const char* e = getenv("MRCNN_GRAPH")) use_graph = atoi(e) != 0;
    if (const char* e = knob_env("MRCNN_FUSE_MASK_TAIL")) fuse_mask_tail = atoi(e) != 0;
    boxes_one_time_init();
    range_flag.alloc(sizeof(int));
    HIP_CHECK(hipMemset(range_flag.p, 0, sizeof(int)));
    nc = (int)file.get_int("num_classes");
    // split modes: the shared-tile K chunks of the long-K 1x1 layers on under-filled grids (single images) and the opt-in fused
    // bottleneck tail need device scratch — owned by this handle from load to destroy (kernels.h: ConvScratch)
    if ((mode == MRCNN_F32S || mode == MRCNN_F32X3) && kind != MRCNN_MODEL_MASK) conv_scratch.alloc();
    if (kind == MRCNN_MODEL_CLASSIFIER) { cls_head.load(file, max_batch, mode); return; }
    if (kind == MRCNN_MODEL_MASK) { mask_head.load(file, max_batch, mode); return; }
    build_maskrcnn();
}

// ------------------------------------------------------------------------------------------------
// the MaskRCNN model: configuration, weights, and the static plan of the trunk
// ------------------------------------------------------------------------------------------------
namespace {

// the five RPN levels P2..P6 of the model's input size: feature-map shape and first anchor
struct Levels {
    int fh[5], fw[5];
    long off[5];
};

// 1. the configuration the artefact carries (defaults: the reference's) and what follows from it
Levels read_config(Model& m)
{
    const MrcwFile& f = m.file;
    m.arch = f.get_string("architecture");
    MRCNN_REQUIRE(m.arch == "resnet101" || m.arch == "resnet50", MRCNN_ERR_UNSUPPORTED, "architecture '%s'", m.arch.c_str());
    m.H = (int)f.get_int("image_height"); m.W = (int)f.get_int("image_width");
    MRCNN_REQUIRE(m.H % 64 == 0 && m.W % 64 == 0 && m.H > 0 && m.W > 0, MRCNN_ERR_SHAPE, "input_image_shape %dx%d must be multiples of 64", m.H, m.W);
    m.na = (int)f.get_int("num_anchors_per_location", 3);
    m.mean[0] = (float)f.get_double("mean_r", 123.7); m.mean[1] = (float)f.get_double("mean_g", 116.8); m.mean[2] = (float)f.get_double("mean_b", 103.9);
    m.pre_nms = (int)f.get_int("ProposalLayer.preNMSMaxProposals", 6000);
    m.max_prop = (int)f.get_int("ProposalLayer.maxProposals", 1000);
    m.prop_nms_thr = (float)f.get_double("ProposalLayer.nmsIOUThreshold", 0.7);
    read_std(f, "ProposalLayer.", m.prop_std);
    m.max_det = (int)f.get_int("DetectionLayer.maxDetections", 100);
    m.det_score_thr = (float)f.get_double("DetectionLayer.scoreThreshold", 0.7);
    m.det_nms_thr = (float)f.get_double("DetectionLayer.nmsIOUThreshold", 0.3);
    read_std(f, "DetectionLayer.", m.det_std);
    m.cls_pool = (int)f.get_int("PyramidROIAlignLayer.classifier.poolSize", 7);
    m.mask_pool = (int)f.get_int("PyramidROIAlignLayer.mask.poolSize", 14);
    m.roi_img_w = f.get_double("PyramidROIAlignLayer.classifier.imageWidth", (double)m.W);
    m.roi_img_h = f.get_double("PyramidROIAlignLayer.classifier.imageHeight", (double)m.H);

    const int strides[5] = {4, 8, 16, 32, 64};
    Levels lv;
    m.A = 0;
    for (int l = 0; l < 5; ++l) {
        lv.fh[l] = (m.H + strides[l] - 1) / strides[l];
        lv.fw[l] = (m.W + strides[l] - 1) / strides[l];
        lv.off[l] = m.A;
        m.A += lv.fh[l] * lv.fw[l] * m.na;
    }
    m.K = m.A < m.pre_nms ? m.A : m.pre_nms;
    return lv;
}

// 2. sub-artefacts from the config singleton (ProposalLayer.swift:68, TimeDistributed*Layer.swift:41/49)
void load_anchors_and_heads(Model& m)
{
    const char* ap = mrcnn_config_get_anchors_path();
    const char* cp = mrcnn_config_get_classifier_path();
    const char* mp = mrcnn_config_get_mask_path();
    MRCNN_REQUIRE(ap, MRCNN_ERR_CONFIG, "MaskRCNNConfig.anchorsURL must be set before the MaskRCNN model is loaded");
    MRCNN_REQUIRE(cp, MRCNN_ERR_CONFIG, "MaskRCNNConfig.compiledClassifierModelURL must be set before the MaskRCNN model is loaded");
    MRCNN_REQUIRE(mp, MRCNN_ERR_CONFIG, "MaskRCNNConfig.compiledMaskModelURL must be set before the MaskRCNN model is loaded");
    {   // anchors.bin: A×4 little-endian float32 (task.py:173-176)
        std::ifstream in(ap, std::ios::binary | std::ios::ate);
        MRCNN_REQUIRE(in.good(), MRCNN_ERR_IO, "cannot open anchors file '%s'", ap);
        const std::streamsize sz = in.tellg();
        MRCNN_REQUIRE(sz == (std::streamsize)m.A * 16, MRCNN_ERR_IO, "anchors file '%s' has %lld bytes, expected %lld (%d anchors x 4 float32)", ap,
                      (long long)sz, (long long)m.A * 16, m.A);
        std::vector<float> h((size_t)m.A * 4);
        in.seekg(0);
        in.read(reinterpret_cast<char*>(h.data()), sz);
        upload(m.anchors, h);
    }
    MrcwFile cf; cf.load(cp);
    MRCNN_REQUIRE(cf.get_string("kind") == "Classifier", MRCNN_ERR_IO, "'%s' is not a Classifier artefact", cp);
    m.cls_head.load(cf, m.max_batch * m.max_prop, m.mode);
    MRCNN_REQUIRE(m.cls_head.nc == m.nc, MRCNN_ERR_IO, "Classifier num_classes %d != %d", m.cls_head.nc, m.nc);
    MrcwFile mf; mf.load(mp);
    MRCNN_REQUIRE(mf.get_string("kind") == "Mask", MRCNN_ERR_IO, "'%s' is not a Mask artefact", mp);
    m.mask_head.load(mf, m.max_batch * m.max_det, m.mode);
    MRCNN_REQUIRE(m.mask_head.nc == m.nc, MRCNN_ERR_IO, "Mask num_classes %d != %d", m.mask_head.nc, m.nc);
}

// 3. trunk weights → m.convs; returns the block letters of the residual stages 2..5
std::vector<std::vector<std::string>> pack_trunk_weights(Model& m)
{
    const MrcwFile& f = m.file;
    const int mode = m.mode;
    auto& convs = m.convs;
    convs["conv1"] = pack_conv1(f, mode);
    std::vector<std::vector<std::string>> blocks(6);
    {
        const int n4 = m.arch == "resnet101" ? 22 : 5;
        blocks[2] = {"a", "b", "c"};
        blocks[3] = {"a", "b", "c", "d"};
        blocks[4] = {"a"};
        for (int i = 0; i < n4; ++i) blocks[4].push_back(std::string(1, (char)('b' + i)));
        blocks[5] = {"a", "b", "c"};
    }
    for (int st = 2; st <= 5; ++st)
        for (auto& b : blocks[st]) {
            const std::string p = std::to_string(st) + b;
            for (const char* br : {"2a", "2b", "2c"}) convs["res" + p + "_branch" + br] = pack_conv_oihw(f, "res" + p + "_branch" + br, "bn" + p + "_branch" + br, mode);
            if (b == "a") convs["res" + p + "_branch1"] = pack_conv_oihw(f, "res" + p + "_branch1", "bn" + p + "_branch1", mode);
        }
    for (const char* n : {"fpn_c5p5", "fpn_c4p4", "fpn_c3p3", "fpn_c2p2", "fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5", "rpn_conv_shared"})
        convs[n] = pack_conv_oihw(f, n, "", mode);
    convs["rpn_heads"] = pack_stacked_1x1(f, {"rpn_class_raw", "rpn_bbox_pred"}, mode);
    const PackedConv& heads = convs["rpn_heads"];
    MRCNN_REQUIRE(heads.Cout == 6 * m.na, MRCNN_ERR_IO, "RPN head width %d != 6*anchors_per_location", heads.Cout);
    if (mode == MRCNN_F16 && heads.Npad == 32 && heads.Cin % 16 == 0) {       // fp16 mode: heads fused into the shared 3x3 layer (kernels_conv3x3_h.hip)
        bneck_pack_frag(nullptr, heads.wgt.p, 32, heads.Cin, m.rpn_head_frag);
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    if (heads.wdtype != heads.dtype && heads.Npad == 32) {                    // split modes: heads fused into the shared 3x3 layer
        conv_halo_pack_head(nullptr, heads.wgt.p, 32, heads.Cin, m.rpn_head_frag);
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    return blocks;
}

// 4. One pass of the activation plan: with real = false it only sizes the arena, with real = true it binds pointers and records the
// ops (lay_out_twice).  Everything a pass leaves in the model is reset HERE, in the constructor, so that the second pass starts
// from what the first one started from.  The ops outlive the builder: their lambdas capture values, never `this`.
struct PlanBuilder {
    Model& m;
    Arena& ar;
    const bool real;
    const int dtype, Bm;
    const Levels& lv;
    const std::vector<std::vector<std::string>>& blocks;
    int g_img, g_zero;
    Tensor4 x;                                                // the running tensor of the backbone
    int g_x = -1;                                             // ... and its group
    Tensor4 Cf[6];
    int g_C[6] = {-1, -1, -1, -1, -1, -1};
    std::vector<BneckTriple> stage_blocks;

    PlanBuilder(Model& model, Arena& arena, bool real_, const Levels& levels, const std::vector<std::vector<std::string>>& blocks_)
        : m(model), ar(arena), real(real_), dtype(model.dtype), Bm(model.max_batch), lv(levels), blocks(blocks_)
    {
        m.trunk_ops.clear();
        m.taps.clear();
        m.sgroups.clear();
        m.sops.clear();
        m.stage_tabs.clear();
        // split groups (engine.h: SplitGroup): g_in / g_out of every convolution; a residual rides in the output's group
        g_img = m.new_split_group("image", true);         // pixel - mean: written by the pre-processing kernel, exponent 0
        g_zero = m.new_split_group("outputs", true);      // logits, box deltas, probabilities: consumed by fp32 arithmetic
    }

    Tensor4 T(int h, int w, int c) { Tensor4 t; t.H = h; t.W = w; t.C = c; t.p = ar.alloc_e((size_t)Bm * h * w * c, dtype); return t; }
    void add(Op op) { if (real) m.trunk_ops.push_back(std::move(op)); }
    // the one ConvDesc maker bound to the model's packs, with the op's own scale / shift copies (null while the arena is being sized)
    ConvDesc desc(const std::string& name, const ConvView& in, const ConvView& out, int stride, int pad, int act, int g_in, int g_out, unsigned retiled)
    {
        const PackedConv* pc = &m.convs.at(name);
        ScaledOp* const so = real ? m.new_scaled_op(pc, g_in, g_out) : nullptr;
        return make_conv_desc(*pc, so ? so->scale.as<float>() : nullptr, so ? so->shift.as<float>() : nullptr, in, out, stride, pad, act, retiled);
    }
    // a layer of the backbone / FPN between two dense tensors: every re-tiled copy its pack holds, an optional residual
    ConvDesc make_desc(const std::string& name, const Tensor4& in, const Tensor4& out, int stride, int pad, int act, const Tensor4* res, int res_shift,
                       int g_in, int g_out)
    {
        ConvDesc d = desc(name, view_of(in), view_of(out), stride, pad, act, g_in, g_out, RETILED_ALL);
        d.group = name.compare(0, 3, "res") == 0 ? 1 : 0;          // conv profile: the backbone subset (C2..C5; conv1 is tagged in stem())
        if (res) set_residual(d, view_of(*res), res_shift);
        return d;
    }
    void conv_op(const std::string& name, const Tensor4& in, const Tensor4& out, int stride, int pad, int act, const Tensor4* res, int res_shift,
                 int g_in, int g_out)
    {
        const ConvDesc d = make_desc(name, in, out, stride, pad, act, res, res_shift, g_in, g_out);
        const size_t per_image = (size_t)out.sB();
        Model* const self = &m;
        add([d, self, g_out, per_image](hipStream_t s, int batch) {
            ConvDesc x = d; x.B = batch; conv_forward(s, x);
            if (self->calib_phase) self->observe_split(s, g_out, d.out, per_image * batch);
        });
    }
    // a bottleneck's tail: branch2b (3x3) and the branch2c (1x1 + shortcut) behind it — one fused launch where the pair
    // qualifies and the grid fills the chip (conv_forward_tail: bit-identical to the two launches), two launches otherwise
    // and while a calibration pass needs the tensor between them
    // dsc: the stage's shortcut convolution (first block) — computed inside branch2c's launch where the pair qualifies (conv_forward),
    // so that its tensor is neither written nor read back; its own launch in a calibration pass (which observes its output)
    // chain (split modes, C2 / C3 / C4's identity pairs): the NEXT block's branch2a rides behind branch2c (conv_forward_chain: bit-identical to its own launch), so
    // the op is held back until the next block has made that layer's description — tail_flush adds it, with or without one
    struct PendingTail { ConvDesc d3, d1, dS; bool has_sc = false; int g_mid = 0, g_out = 0; size_t pm = 0, po = 0; bool open = false; } pending_tail;
    void tail_op(const std::string& n3, const std::string& n1, const Tensor4& in3, const Tensor4& mid, const Tensor4& out, const Tensor4& res,
                 int g_in, int g_mid, int g_out, const ConvDesc* dsc)
    {
        PendingTail& t = pending_tail;
        t.d3 = make_desc(n3, in3, mid, 1, 1, ACT_RELU, nullptr, 0, g_in, g_mid);
        t.d1 = make_desc(n1, mid, out, 1, 0, ACT_RELU, &res, 0, g_mid, g_out);
        t.pm = (size_t)mid.sB(); t.po = (size_t)out.sB();
        t.has_sc = dsc != nullptr;
        t.dS = t.has_sc ? *dsc : ConvDesc();
        t.g_mid = g_mid; t.g_out = g_out;
        t.open = true;
    }
    // dq: the chained layer (the next block's branch2a), g_q its output's group, pq its output's elements per image
    void tail_flush(const ConvDesc* dq = nullptr, int g_q = 0, size_t pq = 0)
    {
        if (!pending_tail.open) return;
        pending_tail.open = false;
        const ConvDesc d3 = pending_tail.d3, d1 = pending_tail.d1, dS = pending_tail.dS;
        const bool has_sc = pending_tail.has_sc, has_q = dq != nullptr;
        const ConvDesc dQ = has_q ? *dq : ConvDesc();
        const int g_mid = pending_tail.g_mid, g_out = pending_tail.g_out;
        const size_t pm = pending_tail.pm, po = pending_tail.po;
        Model* const self = &m;
        add([d3, d1, dS, dQ, has_sc, has_q, self, g_mid, g_out, g_q, pm, po, pq](hipStream_t s, int batch) {
            ConvDesc x3 = d3, x1 = d1, xs = dS, xq = dQ;
            x3.B = x1.B = xs.B = xq.B = batch;
            if (self->calib_phase) {
                if (has_sc) { conv_forward(s, xs); self->observe_split(s, g_out, dS.out, po * batch); }
                conv_forward(s, x3); self->observe_split(s, g_mid, d3.out, pm * batch);
                conv_forward(s, x1); self->observe_split(s, g_out, d1.out, po * batch);
                if (has_q) { conv_forward(s, xq); self->observe_split(s, g_q, dQ.out, pq * batch); }
            } else conv_forward_tail(s, x3, x1, has_sc ? &xs : nullptr, has_q ? &xq : nullptr);
        });
    }

    // fp16 mode — an identity bottleneck (every non-first block of a stage) as ONE persistent launch with both branch tensors on
    // chip (kernels_bneck.hip; bit-identical to the three launches, which conv_bneck_forward runs when the block does not qualify
    // or behind mrcnn_debug_set("conv_bneck", 0)).  The fused form reads halo pixels of x that neighbouring tiles own, so it cannot
    // write in place: such stages ping-pong between two block-output tensors.
    // Round 6: the consecutive identity blocks of a stage are ONE op — where every block takes the fragment-streaming form (C4) they
    // run as ONE launch whose tiles wait for their neighbours' previous block (conv_bneck_stage_forward; bit-identical to the
    // per-block launches, which it falls back to).  The launch reads its per-block operands from a table on the device.
    void bneck_op(const std::string& n_a, const std::string& n_b, const std::string& n_c, const Tensor4& xin, const Tensor4& ta, const Tensor4& tb,
                  const Tensor4& out, int g_in, int g_a, int g_b, int g_out)
    {
        BneckTriple t;
        t.a = make_desc(n_a, xin, ta, 1, 0, ACT_RELU, nullptr, 0, g_in, g_a);
        t.b = make_desc(n_b, ta, tb, 1, 1, ACT_RELU, nullptr, 0, g_a, g_b);
        t.c = make_desc(n_c, tb, out, 1, 0, ACT_RELU, &xin, 0, g_b, g_out);
        stage_blocks.push_back(t);
    }
    void bneck_stage_flush(int tiles_per_image)
    {
        if (stage_blocks.empty()) return;
        const std::vector<BneckTriple> triples = stage_blocks;
        stage_blocks.clear();
        void* tab = nullptr;
        unsigned* done = nullptr;
        bool frag = triples.size() >= 2;
        for (auto& t : triples) frag = frag && t.a.wgt_frag && t.b.wgt_frag && t.c.wgt_frag;
        if (real && frag) {
            const size_t rb = bneck_layer_record_bytes();
            std::vector<unsigned char> h(rb * triples.size());
            for (size_t i = 0; i < triples.size(); ++i)
                bneck_layer_record(h.data() + i * rb, triples[i].a.wgt_frag, triples[i].b.wgt_frag, triples[i].c.wgt_frag, triples[i].a.scale, triples[i].a.shift,
                                   triples[i].b.scale, triples[i].b.shift, triples[i].c.scale, triples[i].c.shift);
            m.stage_tabs.emplace_back(new DevBuf(h.size() + (size_t)Bm * tiles_per_image * sizeof(unsigned)));
            HIP_CHECK(hipMemcpy(m.stage_tabs.back()->p, h.data(), h.size(), hipMemcpyHostToDevice));
            tab = m.stage_tabs.back()->p;
            done = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(tab) + h.size());
        }
        add([triples, tab, done](hipStream_t s, int batch) {
            std::vector<BneckTriple> b = triples;
            for (auto& t : b) t.a.B = t.b.B = t.c.B = batch;
            conv_bneck_stage_forward(s, b.data(), (int)b.size(), tab, done);
        });
    }

    // ---- the steps, in arena order ----------------------------------------------------------------------------------
    void stem()
    {
        const int H = m.H, W = m.W, dt = dtype;
        Model* const self = &m;
        m.d_rgb = (uint8_t*)ar.alloc_b((size_t)Bm * H * W * 3);
        // C1: zero-padded NHWC4 (fp32) / NHWC8 (fp16) staging — 16 B per pixel either way — so the 7×7/2 conv
        // is 7 row-taps of one contiguous 128-B run each; then the 3×3/2 max pool
        const int Hp = H + 6, Wp = W + 6;
        const int pxc = dt == MRCNN_F16 ? 8 : 4;
        void* x0 = ar.alloc_b((size_t)Bm * Hp * Wp * 16 + 256);
        m.stem_in = x0;
        {
            const float m3[3] = {m.mean[0], m.mean[1], m.mean[2]};
            uint8_t* src = m.d_rgb;
            add([src, H, W, m3, x0, dt](hipStream_t s, int batch) { preprocess_forward(s, src, batch, H, W, 3, m3, x0, dt); });
        }
        Tensor4 c1 = T(H / 2, W / 2, 64);
        const int g_c1 = m.new_split_group("C1");                // conv1's output and its max-pooled version (max-pool commutes with the scaling)
        // conv1 omits every re-tiled copy (its pack holds none)
        ConvDesc d = desc("conv1", dense_view(x0, Hp, Wp, pxc), view_of(c1), 2, 0, ACT_RELU, g_img, g_c1, RETILED_NONE);
        d.algo_k = 147;   // 7*7*3 real taps (the packed row is padded to 7*32)
        d.group = 1;
        // split modes: conv1 and the max-pool behind it as ONE persistent launch (kernels_conv_stem.hip) — c1 is then neither
        // written nor read; bit-identical to the two launches, which remain for the other modes and behind "conv_stem" 0
        const size_t per_image = (size_t)c1.sB();
        const int g = g_c1;
        Tensor4 xo = T(H / 4, W / 4, 64);
        const bool stem = conv_stem_eligible(d);
        add([d, self, g, per_image, stem, xo, c1, dt](hipStream_t s, int batch) {
            ConvDesc x = d; x.B = batch;
            if (stem && conv_stem_enabled()) {
                conv_stem_forward(s, x, xo.p, xo.H, xo.W);
                if (self->calib_phase) self->observe_split(s, g, xo.p, (size_t)xo.sB() * batch);     // (max over the pooled tensor = max over c1: every element of c1 lies in a window)
                return;
            }
            conv_forward(s, x);
            if (self->calib_phase) self->observe_split(s, g, d.out, per_image * batch);
            maxpool3x3s2_forward(s, c1.p, batch, c1.H, c1.W, c1.C, xo.p, xo.H, xo.W, dt);
        });
        // trunk taps C1..C5 (parity tests): the arena only grows, so these buffers are not reused by a later layer and still hold
        // their values after predict — C1 the pooled stem output; C{st} the last block output of stage st, which in the fp16 mode's
        // fused stages is stage_main or stage_alt (whichever the last block wrote)
        m.taps["C1"] = {xo.p, xo.sB(), dt, g_c1};
        x = xo;
        g_x = g_c1;
    }

    void residual_stage(int st)
    {
        const int f1s[6] = {0, 0, 64, 128, 256, 512}, f3s[6] = {0, 0, 256, 512, 1024, 2048};
        Tensor4 stage_ta, stage_tb, stage_main, stage_alt;
        bool stage_fused = false, x_is_main = true;
        // every block output of a stage shares ONE group: the blocks add their shortcut in place (res == out)
        const int g_stage = m.new_split_group("C" + std::to_string(st));
        for (auto& b : blocks[st]) {
            const std::string p = std::to_string(st) + b;
            const bool first = b == "a";
            const int stride = (first && st > 2) ? 2 : 1;
            const int oh = x.H / stride, ow = x.W / stride;
            // split modes, C2 / C3: an identity block's branch2a is chained behind the previous block's branch2c (same description, same groups)
            // C4: behind an identity block's branch2c only — the entry block's, which carries the stage's shortcut, keeps its own launch
            const bool chain_q = pending_tail.open && !first && (st == 2 || st == 3 || (st == 4 && !pending_tail.has_sc)) && (m.mode == MRCNN_F32S || m.mode == MRCNN_F32X3);
            if (!chain_q) tail_flush();
            if (first) { stage_ta = T(oh, ow, f1s[st]); stage_tb = T(oh, ow, f1s[st]); }      // the branch tensors are reused by every block of the stage
            if (first && m.mode == MRCNN_F16 && blocks[st].size() > 1 && bneck_geometry_ok(f1s[st], oh, ow)) {
                stage_fused = true;
                stage_alt = T(oh, ow, f3s[st]);
            }
            const int g_a = m.new_split_group("res" + p + "_branch2a"), g_b = m.new_split_group("res" + p + "_branch2b");
            Tensor4 ta = stage_ta;
            Tensor4 tb = stage_tb;
            if (!first && stage_fused) {
                const Tensor4 to = x_is_main ? stage_alt : stage_main;
                bneck_op("res" + p + "_branch2a", "res" + p + "_branch2b", "res" + p + "_branch2c", x, ta, tb, to, g_x, g_a, g_b, g_stage);
                x = to;
                x_is_main = !x_is_main;
                g_x = g_stage;
                continue;
            }
            if (first && m.mode == MRCNN_F16 && stride == 1 && x.C == f1s[st] && f1s[st] == 64 && bneck_geometry_ok(f1s[st], oh, ow)) {
                // fp16 mode, the entry block of C2: branch2a + 2b + 2c AND the shortcut convolution branch1 in one launch (kernels_bneck.hip, FIRST
                // form; bit-identical to the four launches, which conv_bneck_first_forward runs where the block does not qualify)
                const Tensor4 sc1 = T(oh, ow, f3s[st]);         // the shortcut tensor of the four-launch form (unused by the fused one)
                const Tensor4 out1 = T(oh, ow, f3s[st]);
                const ConvDesc da = make_desc("res" + p + "_branch2a", x, ta, 1, 0, ACT_RELU, nullptr, 0, g_x, g_a);
                const ConvDesc db = make_desc("res" + p + "_branch2b", ta, tb, 1, 1, ACT_RELU, nullptr, 0, g_a, g_b);
                const ConvDesc ds = make_desc("res" + p + "_branch1", x, sc1, 1, 0, ACT_NONE, nullptr, 0, g_x, g_stage);
                const ConvDesc dc = make_desc("res" + p + "_branch2c", tb, out1, 1, 0, ACT_RELU, &sc1, 0, g_b, g_stage);
                add([da, db, dc, ds](hipStream_t s, int batch) {
                    ConvDesc a = da, b = db, c = dc, e = ds;
                    a.B = b.B = c.B = e.B = batch;
                    conv_bneck_first_forward(s, a, b, c, e);
                });
                x = out1;
                stage_main = out1;
                g_x = g_stage;
                continue;
            }
            if (chain_q) {
                const ConvDesc dq = make_desc("res" + p + "_branch2a", x, ta, stride, 0, ACT_RELU, nullptr, 0, g_x, g_a);
                tail_flush(&dq, g_a, (size_t)ta.sB());
            } else conv_op("res" + p + "_branch2a", x, ta, stride, 0, ACT_RELU, nullptr, 0, g_x, g_a);
            Tensor4 sc = x;
            ConvDesc dsc;
            if (first) {
                sc = T(oh, ow, f3s[st]);
                dsc = make_desc("res" + p + "_branch1", x, sc, stride, 0, ACT_NONE, nullptr, 0, g_x, g_stage);
            }
            // The block's output overwrites its shortcut IN PLACE (branch2c reads a residual element and writes the output
            // element at the same address, from the same thread; nothing reads the shortcut afterwards): a stage then cycles
            // through x + two branch tensors — 200 MB for C4 at batch 8, inside the 256 MB Infinity Cache — instead of
            // streaming a fresh 134 MB tensor per block through HBM.
            Tensor4 to = sc;
            tail_op("res" + p + "_branch2b", "res" + p + "_branch2c", ta, tb, to, sc, g_a, g_b, g_stage, first ? &dsc : nullptr);
            x = to;
            if (first) stage_main = to;
            g_x = g_stage;
        }
        tail_flush();
        bneck_stage_flush((x.H / (f1s[st] == 256 ? 8 : 16)) * (x.W / 16));
        Cf[st] = x;
        g_C[st] = g_stage;
        m.taps["C" + std::to_string(st)] = {x.p, x.sB(), dtype, g_stage};
    }

    // FPN: lateral 1×1 (+ nearest 2× upsample of the level above, fused as a shifted residual), then 3×3
    void fpn()
    {
        Tensor4 L5 = T(Cf[5].H, Cf[5].W, 256), L4 = T(Cf[4].H, Cf[4].W, 256), L3 = T(Cf[3].H, Cf[3].W, 256), L2 = T(Cf[2].H, Cf[2].W, 256);
        const int g_L = m.new_split_group("fpn_lateral");           // L5..L2 add each other (top-down): one group
        conv_op("fpn_c5p5", Cf[5], L5, 1, 0, ACT_NONE, nullptr, 0, g_C[5], g_L);
        conv_op("fpn_c4p4", Cf[4], L4, 1, 0, ACT_NONE, &L5, 1, g_C[4], g_L);
        conv_op("fpn_c3p3", Cf[3], L3, 1, 0, ACT_NONE, &L4, 1, g_C[3], g_L);
        conv_op("fpn_c2p2", Cf[2], L2, 1, 0, ACT_NONE, &L3, 1, g_C[2], g_L);
        const Tensor4 Ls[4] = {L2, L3, L4, L5};
        const char* pn[4] = {"fpn_p2", "fpn_p3", "fpn_p4", "fpn_p5"};
        const char* tn[4] = {"P2", "P3", "P4", "P5"};
        for (int l = 0; l < 4; ++l) {
            m.P[l] = T(Ls[l].H, Ls[l].W, 256);
            m.g_P[l] = m.new_split_group(tn[l]);
            conv_op(pn[l], Ls[l], m.P[l], 1, 1, ACT_NONE, nullptr, 0, g_L, m.g_P[l]);
            m.taps[tn[l]] = {m.P[l].p, m.P[l].sB(), dtype, m.g_P[l]};
            MRCNN_REQUIRE(m.P[l].H == lv.fh[l] && m.P[l].W == lv.fw[l], MRCNN_ERR_SHAPE, "pyramid level %d shape mismatch", l + 2);
        }
    }

    // RPN on P2..P6 (P6 = P5 sub-sampled by 2: read in place through doubled strides)
    void rpn()
    {
        const int A = m.A, na = m.na, mode = m.mode;
        Model* const self = &m;
        m.rpn_logits = ar.alloc_f((size_t)Bm * A * 2);
        m.rpn_probs = ar.alloc_f((size_t)Bm * A * 2);
        m.rpn_deltas = ar.alloc_f((size_t)Bm * A * 4);
        m.taps["rpn_probs"] = {m.rpn_probs, (long)A * 2, MRCNN_F32};
        m.taps["rpn_deltas"] = {m.rpn_deltas, (long)A * 4, MRCNN_F32};
        // the shared layer's 512-channel tensor: ONE buffer, sized for the largest level, reused level after level on the model's stream
        // (round 5's per-level copies served the level-parallel region, measured slower and removed in round 6: profiles/r05_level_parallel_ab.txt)
        void* const rpn_feat = ar.alloc_e((size_t)Bm * lv.fh[0] * lv.fw[0] * 512, dtype);
        const PackedConv* hc = &m.convs.at("rpn_heads");
        for (int l = 0; l < 5; ++l) {
            const int fh = lv.fh[l], fw = lv.fw[l];
            const Tensor4& src = m.P[l < 4 ? l : 3];
            const int sub = l < 4 ? 1 : 2;
            m.g_rpn[l] = m.new_split_group("rpn_feat_P" + std::to_string(l + 2));
            const ConvView feat = dense_view(rpn_feat, fh, fw, 512);
            // the shared 3x3 layer passes its halo and 3x3-fp16 copies, not wgt_frag (its pack holds none)
            const ConvDesc d = desc("rpn_conv_shared", {src.p, fh, fw, src.sB(), (long)sub * src.W * src.C, (long)sub * src.C}, feat, 1, 1, ACT_RELU,
                                    m.g_P[l < 4 ? l : 3], m.g_rpn[l], RETILED_HALO | RETILED_C3H);
            // the separate head launch undoes the exponent in its scale; the box path consumes fp32 (ProposalLayer.swift:108-109)
            ConvDesc e = desc("rpn_heads", feat, {m.rpn_logits + lv.off[l] * 2, fh, fw, (long)A * 2, (long)fw * 2 * na, (long)2 * na}, 1, 0, ACT_NONE,
                              m.g_rpn[l], g_zero, RETILED_NONE);
            e.out_f32 = 1;
            e.out2 = m.rpn_deltas + lv.off[l] * 4; e.out2_sP = 4 * na; e.out2_sB = (long)A * 4; e.n_split = 2 * na;
            // Levels whose geometry qualifies (a property of the level, not of the batch: P2..P4 at 1024²) run the two heads INSIDE
            // the shared 3x3 layer's epilogue: the 512-channel tensor — 1.07 GB at P2, batch 8 — is neither
            // written nor read back, and the head launches disappear.  Switched off with the halo kernel itself: the two launches.
            ConvDesc f = d;
            f.B = 1;
            f.head_w = m.rpn_head_frag.p; f.head_bias = hc->shift.as<float>();
            f.head_out = m.rpn_logits + lv.off[l] * 2; f.head_out_sP = 2 * na; f.head_out_sB = (long)A * 2;
            f.head_out2 = m.rpn_deltas + lv.off[l] * 4; f.head_out2_sP = 4 * na; f.head_out2_sB = (long)A * 4;
            f.head_split = 2 * na; f.head_cols = 6 * na;
            // fp16 mode: the same fusion on the halo-tile kernel of kernels_conv3x3_h.hip, on the levels with >= 16384 pixels per image (P2, P3 at 1024^2 — P4's 16 tiles per image would leave half the chip idle at batch 8:
            // a property of the level, like the split modes' rule); bit-identical to that kernel followed by the separate head launch
            const bool fuse16 = mode == MRCNN_F16 && m.rpn_head_frag.p && d.wgt_c3h && (long)fh * fw >= 16384 && conv3x3h_eligible(f);
            const bool fuse = fuse16 || (mode != MRCNN_F16 && m.rpn_head_frag.p && d.wgt_halo && conv_halo_head_eligible(f));
            const int g_r = m.g_rpn[l];
            const size_t per_image = (size_t)fh * fw * 512;
            add([d, e, f, fuse, fuse16, self, g_r, per_image](hipStream_t s, int batch) {
                // (a calibration pass needs the 512-channel tensor: it runs the two-launch form)
                const int c3h = conv_c3h_mode();
                if (fuse && (fuse16 ? (c3h == 1 || c3h == 2) : conv_halo_enabled()) && !self->calib_phase) {
                    ConvDesc x = f; x.B = batch;
                    x.head_mul = ldexpf(1.0f, -self->sgroups[(size_t)g_r].exp);       // the fused heads see 2^e * relu(...): undone on their sums (exact)
                    conv_forward(s, x);
                    return;
                }
                ConvDesc x = d; x.B = batch;
                x.prefer_c3h = fuse16 && c3h == 3;               // (the fused form's own 3x3 kernel followed by the separate head launch: bit-identical to the fusion)
                conv_forward(s, x);
                if (self->calib_phase) self->observe_split(s, g_r, d.out, per_image * batch);
                ConvDesc y = e; y.B = batch; conv_forward(s, y);
            });
        }
        float* lg = m.rpn_logits; float* pr = m.rpn_probs; const long per = A;
        add([lg, pr, per](hipStream_t s, int batch) { softmax_pairs_forward(s, lg, pr, per * batch); });
    }

    // box and mask buffers, workspaces, and the heads' groups
    void heads()
    {
        const int max_prop = m.max_prop, max_det = m.max_det, cls_pool = m.cls_pool, mask_pool = m.mask_pool, dt = dtype;
        m.rois = ar.alloc_f((size_t)Bm * max_prop * 4);
        m.pooled = ar.alloc_e((size_t)Bm * max_prop * cls_pool * cls_pool * 256, dt);
        m.cls6 = ar.alloc_f((size_t)Bm * max_prop * 6);
        m.detections = ar.alloc_f((size_t)Bm * max_det * 6);
        m.pooled_mask = ar.alloc_e((size_t)Bm * max_det * mask_pool * mask_pool * 256, dt);
        m.mask_out = ar.alloc_f((size_t)Bm * max_det * 4 * mask_pool * mask_pool);
        m.taps["rois"] = {m.rois, (long)max_prop * 4, MRCNN_F32};
        m.g_pooled = m.new_split_group("pooled");
        m.g_pooled_mask = m.new_split_group("pooled_mask");
        m.taps["pooled"] = {m.pooled, (long)max_prop * cls_pool * cls_pool * 256, dt, m.g_pooled};
        m.taps["cls6"] = {m.cls6, (long)max_prop * 6, MRCNN_F32};
        m.taps["detections"] = {m.detections, (long)max_det * 6, MRCNN_F32};
        m.taps["pooled_mask"] = {m.pooled_mask, (long)max_det * mask_pool * mask_pool * 256, dt, m.g_pooled_mask};
        m.taps["mask"] = {m.mask_out, (long)max_det * 4 * mask_pool * mask_pool, MRCNN_F32};
        void* pws = ar.alloc_b(ProposalWorkspace::bytes(Bm, m.A, m.K, max_prop));
        void* dws = ar.alloc_b(DetectionWorkspace::bytes(Bm, max_prop, max_det));
        m.msel_ws.flags = (int32_t*)ar.alloc_b((size_t)Bm * max_det * 4);
        m.msel_ws.mapping = (int32_t*)ar.alloc_b((size_t)Bm * max_det * 4);
        m.msel_ws.kept = (int32_t*)ar.alloc_b((size_t)Bm * 4);
        m.msel_ws.sel_cid = (int32_t*)ar.alloc_b((size_t)Bm * max_det * 4);
        m.mask_partial = ar.alloc_f((size_t)Bm * max_det * 4 * mask_pool * mask_pool * (256 / 64));        // (up to four partial sums per output pixel: conv_sel_part_cols)
        if (!real) return;
        m.prop_ws.bind(pws, Bm, m.A, m.K, max_prop);
        m.det_ws.bind(dws, Bm, max_prop, max_det);
        // the heads' layers: pooled → h1 → h2 → logits (0);  pooled_mask → t1..t4 → deconvolution output (0: its consumer is an fp32 dot)
        ClassifierHead& ch = m.cls_head;
        MaskHead& mh = m.mask_head;
        ch.grp[0] = m.g_pooled; ch.grp[1] = m.new_split_group("cls_h1"); ch.grp[2] = m.new_split_group("cls_h2");
        mh.grp[0] = m.g_pooled_mask;
        for (int i = 1; i <= 4; ++i) mh.grp[i] = m.new_split_group("mask_t" + std::to_string(i));
        for (int i = 0; i < 3; ++i) { ch.sop[i].g_in = ch.grp[i]; ch.sop[i].g_out = i < 2 ? ch.grp[i + 1] : g_zero; }
        for (int i = 0; i < 5; ++i) { mh.sop[i].g_in = mh.grp[i]; mh.sop[i].g_out = i < 4 ? mh.grp[i + 1] : g_zero; }
        Model* const self = &m;
        ch.observe = [self](hipStream_t s, int g, const void* x, size_t n) { if (self->calib_phase) self->observe_split(s, g, x, n); };
        mh.observe = ch.observe;
    }
};

// 5. the exponents stored with the artefact, or the one the measurement override names
void apply_initial_exponents(Model& m)
{
    m.calib_buf.alloc(m.sgroups.size() * 32);
    HIP_CHECK(hipMemset(m.calib_buf.p, 0, m.sgroups.size() * 32));
    const bool split_mode = m.mode == MRCNN_F32S || m.mode == MRCNN_F32X3;
    if (split_mode) {
        // exponents stored with the artefact (convert.py --calibrate: "split_exp.<group>" metadata): the drop-in prediction() needs no call
        int found = 0;
        for (auto& g : m.sgroups) {
            const auto it = m.file.ints.find("split_exp." + g.name);
            if (it == m.file.ints.end() || g.fixed) continue;
            MRCNN_REQUIRE(it->second >= -60 && it->second <= 60, MRCNN_ERR_IO, "stored split exponent of group '%s' out of range", g.name.c_str());
            g.exp = (int)it->second;
            ++found;
        }
        if (found) { m.apply_split_exponents(); m.split_calibrated = true; m.exponents_from_artefact = true; }
    }
    if (const char* e = knob_env("MRCNN_SPLIT_EXP")) {          // measurement / tests: one exponent for every non-fixed group (split modes only)
        if (split_mode) {
            for (auto& g : m.sgroups) if (!g.fixed) g.exp = atoi(e);
            m.apply_split_exponents();
        } else fprintf(stderr, "libmaskrcnn_hip: MRCNN_SPLIT_EXP ignored: compute mode %d carries no split exponents\n", m.mode);
    }
}

}  // namespace

void Model::build_maskrcnn()
{
    const Levels lv = read_config(*this);
    load_anchors_and_heads(*this);
    const std::vector<std::vector<std::string>> blocks = pack_trunk_weights(*this);
    // the activation plan: the first pass sizes the arena, the second binds pointers and records the ops
    lay_out_twice(arena, [&](Arena& ar, bool real) {
        PlanBuilder p(*this, ar, real, lv, blocks);
        p.stem();
        for (int st = 2; st <= 5; ++st) p.residual_stage(st);
        p.fpn();
        p.rpn();
        p.heads();
    });
    apply_initial_exponents(*this);
    taps["cls_probs"] = {cls_head.probs, (long)max_prop * nc, MRCNN_F32};
    taps["cls_bbox"] = {cls_head.bbox, (long)max_prop * nc * 4, MRCNN_F32};
}

}  // namespace mrcnn
