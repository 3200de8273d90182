"""GPU parity of the fused engine (MaskRCNN.predict) against the CPU oracle, stage by stage.

The trunk (fp32 MFMA convolutions) is compared with the torch-CPU fp32 network within a stated
tolerance; every later stage is fed THE GPU'S OWN tap of its input and must then agree with the
oracle bit-exactly where it is index/box arithmetic (top-k order, proposals, ROIAlign samples,
class ids, detections) and within tolerance where convolutions are involved (box head, mask head).
This is how "bit-exact for top-k indices and class labels, fp32 tolerance elsewhere" is pinned
without requiring two different summation orders to round identically through 100+ layers.
"""
import os

import numpy as np
import pytest

from conftest import rand_images, make_model_dir

pytestmark = pytest.mark.gpu

TRUNK_RTOL = 5e-4   # max |gpu - cpu| / max |cpu| per tensor, fp32 vs fp32 with different summation order


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def _nhwc_to_chw(x, h, w, c):
    return np.ascontiguousarray(x.reshape(h, w, c).transpose(2, 0, 1))


def _check_stages(pkg, orc, om, m, cfg, images, b, check_trunk=True, trunk=None, f16=False, tb=None):
    """f16: the engine runs fp16 activations/filters with fp32 accumulation (BASELINE configs[3]).  The
    convolutional stages are then compared with the fp32 CPU network at fp16-level tolerances, while
    every index/box stage stays bit-exact on the GPU's own taps (ROIAlign: same fp32 arithmetic on the
    widened fp16 samples, rounded once to fp16)."""
    H, W = cfg.image_height, cfg.image_width
    conv_tol = 4e-2 if f16 else TRUNK_RTOL
    prob_tol = 4e-2 if f16 else 5e-4
    rnd = (lambda x: x.astype(np.float16).astype(np.float32)) if f16 else (lambda x: x)
    shapes = cfg.feature_shapes()
    A = cfg.num_anchors()
    # ---- trunk ---------------------------------------------------------------------------------
    P = [_nhwc_to_chw(m.read_tensor(f"P{l + 2}", b), shapes[l][0], shapes[l][1], 256) for l in range(4)]
    probs = m.read_tensor("rpn_probs", b).reshape(A, 2)
    deltas = m.read_tensor("rpn_deltas", b).reshape(A, 4)
    if check_trunk:
        pyr, oprobs, odeltas = trunk
        tb = b if tb is None else tb            # row of `trunk` that holds image b (the oracle may have run on a subset)
        for l in range(4):
            assert _rel(P[l], pyr[l][tb]) < conv_tol, f"P{l + 2}"
        assert _rel(deltas, odeltas[tb]) < conv_tol
        assert np.abs(probs - oprobs[tb]).max() < prob_tol
    # ---- ProposalLayer on the GPU's RPN outputs: bit-exact ---------------------------------------
    K = min(A, cfg.pre_nms_max_proposals)
    want_rois, dbg = om.proposals(probs, deltas, debug=True)
    np.testing.assert_array_equal(m.read_tensor("topk_idx", b).astype(np.int64), dbg["topk_idx"].astype(np.int64))
    np.testing.assert_array_equal(m.read_tensor("boxes_sorted", b).reshape(K, 4), dbg["boxes"])
    rois = m.read_tensor("rois", b).reshape(cfg.max_proposals, 4)
    np.testing.assert_array_equal(rois, want_rois)
    assert int(m.read_tensor("keep_count", b)[0]) == dbg["count"]
    # ---- PyramidROIAlign (7×7) on the GPU's pyramid + rois: bit-exact -----------------------------
    ps = cfg.classifier_pool_size
    pooled = m.read_tensor("pooled", b).reshape(cfg.max_proposals, ps, ps, 256).transpose(0, 3, 1, 2)
    np.testing.assert_array_equal(pooled, rnd(om.roi_align(rois, P, ps)))
    # ---- box head: tolerance; post-processing bit-exact on the GPU's probabilities ---------------
    gp = m.read_tensor("cls_probs", b).reshape(cfg.max_proposals, cfg.num_classes)
    gb = m.read_tensor("cls_bbox", b).reshape(cfg.max_proposals, cfg.num_classes * 4)
    _, op, ob = om.classify(np.ascontiguousarray(pooled))
    assert np.abs(gp - op).max() < prob_tol
    assert _rel(gb, ob) < conv_tol
    cls6 = m.read_tensor("cls6", b).reshape(cfg.max_proposals, 6)
    np.testing.assert_array_equal(cls6, orc.classifier_postprocess(gp, gb))
    # ---- DetectionLayer on the GPU's rois + cls6: bit-exact ---------------------------------------
    det = m.read_tensor("detections", b).reshape(cfg.max_detections, 6)
    np.testing.assert_array_equal(det, om.detect(rois, cls6))
    # ---- PyramidROIAlign (14×14) on the detections: bit-exact -------------------------------------
    pm = cfg.mask_pool_size
    pooled_m = m.read_tensor("pooled_mask", b).reshape(cfg.max_detections, pm, pm, 256).transpose(0, 3, 1, 2)
    samples = om.roi_align(det, P, pm)            # fp32 samples; the fp16 engine stores them rounded once
    np.testing.assert_array_equal(pooled_m, rnd(samples))
    # removeZeros predicate: decided on the fp32 samples in every mode (TimeDistributedClassifierLayer.swift:116-127)
    flags = m.read_tensor("mask_row_flags", b).astype(np.int64)
    want_flags = np.zeros(cfg.max_detections, np.int64)
    want_flags[orc.mask_valid_rows(samples)] = 1
    np.testing.assert_array_equal(flags, want_flags)
    # ---- mask head: same write set, values within 3e-4 --------------------------------------------
    mask = m.read_tensor("mask", b).reshape(cfg.max_detections, 4 * pm * pm)
    want = om.masks(np.ascontiguousarray(pooled_m), det, valid_from=samples)
    np.testing.assert_array_equal(mask == 0, want == 0)
    assert np.abs(mask - want).max() < (3e-2 if f16 else 3e-4)
    return det, mask


def test_engine_small_staged(pkg, orc, small_model):
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    om = load_oracle_model(d)
    B = 3
    m = models.load_maskrcnn(d, max_batch=B)
    images = rand_images(B, cfg.image_height, cfg.image_width, seed=1)
    det, mask = m.predict(images)
    assert det.shape == (B, cfg.max_detections, 6) and mask.shape == (B, cfg.max_detections, 28, 28)
    trunk = om.trunk(images)
    n_det = []
    for b in range(B):
        d_b, m_b = _check_stages(pkg, orc, om, m, cfg, images, b, True, trunk)
        np.testing.assert_array_equal(det[b], d_b)
        np.testing.assert_array_equal(mask[b].reshape(cfg.max_detections, -1), m_b)
        n_det.append(int((d_b[:, 5] > 0).sum()))
    assert max(n_det) > 0, "synthetic weights produced no detections: the heads were not exercised"


def test_engine_batch_independence(pkg, small_model):
    """Per-image results do not depend on the batch they ride in (the multi-GPU sharding contract)."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=4)
    images = rand_images(4, cfg.image_height, cfg.image_width, seed=3)
    det, mask = m.predict(images)
    for b in range(4):
        d1, m1 = m.predict(images[b:b + 1])
        np.testing.assert_array_equal(d1[0], det[b])
        np.testing.assert_array_equal(m1[0], mask[b])
    # reference-shaped single-image call and the decoder
    r = m.prediction(images[0])
    np.testing.assert_array_equal(r["detections"], det[0])
    dets = pkg.Detection.detectionsFromFeatureValue(r["detections"], r["mask"])
    assert len(dets) == int((det[0][:, 5] > 0.7).sum())
    for dd in dets:
        assert dd.mask.shape == (28, 28) and dd.mask.dtype == np.uint8


def test_engine_device_tensors(pkg, small_model):
    import torch
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=2)
    images = rand_images(2, cfg.image_height, cfg.image_width, seed=5)
    det_h, mask_h = m.predict(images)
    det_d, mask_d = m.predict(torch.from_numpy(images).cuda())
    np.testing.assert_array_equal(det_d.cpu().numpy(), det_h)
    np.testing.assert_array_equal(mask_d.cpu().numpy(), mask_h)
    m.enable_timing(True)
    m.predict(images)
    ms = m.stage_ms()
    assert all(v >= 0 for v in ms.values()) and ms["Trunk"] > 0


def test_engine_errors(pkg, small_model, tmp_path):
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=1)
    with pytest.raises(Exception) as e:
        m.predict(rand_images(1, 64, 64))
    assert "expects" in str(e.value)
    with pytest.raises(Exception):
        m.predict(rand_images(2, cfg.image_height, cfg.image_width))       # batch > max_batch
    with pytest.raises(Exception) as e:
        models.MaskRCNN(os.path.join(d, "Classifier.mrcw"))                 # wrong artefact kind
    assert "expected MaskRCNN" in str(e.value)
    bad = tmp_path / "bad.mrcw"
    bad.write_bytes(b"nope")
    with pytest.raises(Exception):
        models.Classifier(str(bad))
    pkg.MaskRCNNConfig.defaultConfig().anchorsURL = str(tmp_path / "missing.bin")
    with pytest.raises(Exception) as e:
        models.MaskRCNN(os.path.join(d, "MaskRCNN.mrcw"))
    assert "anchors" in str(e.value)


def test_engine_loads_converted_artefacts(pkg, small_model, weights_mod, tmp_path):
    """`maskrcnn convert` products (from a Keras-layout checkpoint dict) drive the engine exactly like the
    artefacts they were derived from — with fp16 tensors (task.py:90) and with fp32 tensors in the file."""
    il = __import__("importlib")
    models, conv = il.import_module("mask-rcnn-coreml_amd.models"), il.import_module("mask-rcnn-coreml_amd.convert")
    anchors = il.import_module("mask-rcnn-coreml_amd.anchors")
    d, cfg = small_model
    images = rand_images(2, cfg.image_height, cfg.image_width, seed=9)
    det0, mask0 = models.load_maskrcnn(d, max_batch=2).predict(images)
    keras = {}
    for kind in ("MaskRCNN", "Classifier", "Mask"):
        _, tensors = weights_mod.read_mrcw(os.path.join(d, f"{kind}.mrcw"))
        for n, a in tensors.items():
            keras[conv.keras_name(n)] = np.ascontiguousarray(conv.to_keras_layout(n, a.astype(np.float32)))
    for wd in ("f16", "f32"):
        out = tmp_path / wd
        out.mkdir()
        converted, unused = conv.convert_tensors(keras, cfg, weights_dtype=wd)
        assert not unused
        for kind, (meta, tensors) in converted.items():
            weights_mod.write_mrcw(str(out / f"{kind}.mrcw"), meta, tensors)
        anchors.write_anchors_bin(str(out / "anchors.bin"), cfg)
        det, mask = models.load_maskrcnn(str(out), max_batch=2).predict(images)
        np.testing.assert_array_equal(det, det0)
        np.testing.assert_array_equal(mask, mask0)
    assert (det0[:, :, 5] > 0).any()


def test_engine_resnet101_256(pkg, orc, tmp_path_factory, weights_mod):
    """ResNet-101 (23 C4 blocks) at 256² with the default 81 classes, batch 2."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "r101", architecture="resnet101",
                            input_image_shape=(256, 256, 3), pre_nms_max_proposals=1000, max_proposals=128,
                            max_detections=32)
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=2)
    images = rand_images(2, 256, 256, seed=7)
    m.predict(images)
    trunk = om.trunk(images)
    for b in range(2):
        _check_stages(pkg, orc, om, m, cfg, images, b, True, trunk)


@pytest.mark.parametrize("mode", ["f32x3", "f32"])
def test_engine_config3_resnet50_1024(pkg, orc, tmp_path_factory, weights_mod, mode):
    """BASELINE configs[2] per-GPU slice: ResNet50+FPN at 1024² (C4 = 6 blocks), batch 2 — in the headline mode (f32x3,
    the mode profiles/*_bench_n1_resnet50.json is quoted in) and in the fp32-MFMA mode."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "r50full" + mode, architecture="resnet50")
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype=mode)
    images = rand_images(2, 1024, 1024, seed=11)
    m.predict(images)
    trunk = om.trunk(images[:1])
    _check_stages(pkg, orc, om, m, cfg, images, 0, True, trunk)
    _check_stages(pkg, orc, om, m, cfg, images, 1, False)


@pytest.mark.parametrize("mode", ["f32x3", "f32"])
def test_engine_config5_1536_two_classes(pkg, orc, tmp_path_factory, weights_mod, mode):
    """BASELINE configs[4]: 1536×1536, num_classes = 2, pre_nms 12000 (NMS / ROIAlign stress):
    A = 589 248 anchors, pyramid 384²..24², every stage after the trunk bit-exact on the GPU's taps — in the headline
    mode (f32x3, the mode profiles/*_config5_1536.json is quoted in) and in the fp32-MFMA mode."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "c5" + mode, architecture="resnet101",
                            input_image_shape=(1536, 1536, 3), num_classes=2, pre_nms_max_proposals=12000)
    assert cfg.num_anchors() == 589248
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=1, compute_dtype=mode)
    images = rand_images(1, 1536, 1536, seed=13)
    m.predict(images)
    trunk = om.trunk(images)
    _check_stages(pkg, orc, om, m, cfg, images, 0, True, trunk)


def test_engine_fp16_small_staged(pkg, orc, small_model):
    """compute_dtype = f16 (fp16 MFMA, fp32 accumulate) on the small model, batch 2."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype="f16")
    assert m.get_int("compute_dtype") == 2
    images = rand_images(2, cfg.image_height, cfg.image_width, seed=1)
    det, mask = m.predict(images)
    trunk = om.trunk(images)
    for b in range(2):
        d_b, m_b = _check_stages(pkg, orc, om, m, cfg, images, b, True, trunk, f16=True)
        np.testing.assert_array_equal(det[b], d_b)
    # per-image results independent of the batch
    d1, m1 = m.predict(images[1:2])
    np.testing.assert_array_equal(d1[0], det[1])
    np.testing.assert_array_equal(m1[0], mask[1])


def test_engine_config4_fp16_full_size(pkg, orc, tmp_path_factory, weights_mod):
    """BASELINE configs[3] per-GPU slice: ResNet101+FPN, 1024², fp16 MFMA convs (batch 2 here)."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "full16", architecture="resnet101")
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype="f16")
    images = rand_images(2, 1024, 1024, seed=1)
    m.predict(images)
    trunk = om.trunk(images[:1])
    d0, _ = _check_stages(pkg, orc, om, m, cfg, images, 0, True, trunk, f16=True)
    _check_stages(pkg, orc, om, m, cfg, images, 1, False, f16=True)
    assert int(m.read_tensor("keep_count", 0)[0]) == cfg.max_proposals
    assert int((d0[:, 5] > 0).sum()) == cfg.max_detections


def test_engine_full_size_one_image(pkg, orc, tmp_path_factory, weights_mod):
    """BASELINE config: ResNet-101 + FPN, 1024², 81 classes, preNMS 6000, 1000 proposals, 100
    detections — one image, every stage after the trunk bit-exact on the GPU's taps; the trunk
    itself against torch-CPU fp32."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "full", architecture="resnet101")
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=1)
    images = rand_images(1, 1024, 1024, seed=1)
    det, mask = m.predict(images)
    trunk = om.trunk(images)
    d0, _ = _check_stages(pkg, orc, om, m, cfg, images, 0, True, trunk)
    # the synthetic "forced full load" weights must actually load the data-dependent stages
    assert int(m.read_tensor("keep_count", 0)[0]) == cfg.max_proposals
    assert int((d0[:, 5] > 0).sum()) == cfg.max_detections


@pytest.mark.parametrize("mode", ["f32s", "f32x3"])
def test_engine_f32s_split_mode(pkg, orc, small_model, weights_mod, tmp_path, mode):
    """MRCNN_F32S / MRCNN_F32X3: fp32 tensors, convolutions as two / three fp16 MFMA passes over a split of the activations.
    Same staged parity as the fp32 engine AT THE SAME fp32 TOLERANCES, per-image batch independence, agreement
    with the exact-fp32 engine to a few 1e-6, and refusal of artefacts whose filters are not fp16-representable."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    om = load_oracle_model(d)
    B = 3
    images = rand_images(B, cfg.image_height, cfg.image_width, seed=1)
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype=mode)
    assert m.get_int("compute_dtype") == {"f32s": 5, "f32x3": 6}[mode]
    det, mask = m.predict(images)
    trunk = om.trunk(images)
    for b in range(B):
        d_b, m_b = _check_stages(pkg, orc, om, m, cfg, images, b, True, trunk)          # fp32 tolerances
        np.testing.assert_array_equal(det[b], d_b)
        np.testing.assert_array_equal(mask[b].reshape(cfg.max_detections, -1), m_b)
    d1, m1 = m.predict(images[2:3])
    np.testing.assert_array_equal(d1[0], det[2])
    np.testing.assert_array_equal(m1[0], mask[2])
    # against the exact-fp32 engine: the pyramid after ~50 convolutions agrees to ~3e-6 of its range
    m32 = models.load_maskrcnn(d, max_batch=B)
    m32.predict(images)
    for name in ("P2", "P3", "P4", "P5", "rpn_deltas"):
        x, y = m32.read_tensor(name, 1), m.read_tensor(name, 1)
        assert _rel(y, x) < (2e-5 if mode == "f32s" else 4e-6), name      # three parts: only the summation order differs
    # and to the oracle it is as close as the fp32 engine is (both sit at summation-order noise)
    pyr = trunk[0]
    h, w = cfg.feature_shapes()[0]
    e32 = _rel(_nhwc_to_chw(m32.read_tensor("P2", 1), h, w, 256), pyr[0][1])
    e32s = _rel(_nhwc_to_chw(m.read_tensor("P2", 1), h, w, 256), pyr[0][1])
    assert e32s < max(4 * e32, 2e-5), (e32, e32s)
    # genuine fp32 filters cannot be split exactly: refused with a message, never silently rounded
    bad = tmp_path / "fp32w"
    bad.mkdir()
    for kind in ("MaskRCNN", "Classifier", "Mask"):
        meta, tensors = weights_mod.read_mrcw(os.path.join(d, f"{kind}.mrcw"))
        t32 = {k: v.astype(np.float32) for k, v in tensors.items()}
        if kind == "MaskRCNN":
            t32["res2a_branch2a/kernel"] = t32["res2a_branch2a/kernel"] * np.float32(1.0001)
        weights_mod.write_mrcw(str(bad / f"{kind}.mrcw"), meta, t32)
    __import__("importlib").import_module("mask-rcnn-coreml_amd.anchors").write_anchors_bin(str(bad / "anchors.bin"), cfg)
    models.load_maskrcnn(str(bad), max_batch=1)                                           # fine in fp32
    with pytest.raises(Exception, match="not fp16-representable"):
        models.load_maskrcnn(str(bad), max_batch=1, compute_dtype=mode)
    pkg.MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(d, "anchors.bin")


@pytest.mark.parametrize("mode", ["f32", "f32s", "f32x3", "f16"])
def test_engine_sparse_outcomes(pkg, orc, weights_mod, tmp_path, mode):
    """Plain He-init weights (no forced load): the RPN soft-max sits near 0.5, NMS keeps fewer than maxProposals, almost no
    row passes the 0.7 score filter — the zero-padding / short-count paths of every stage, and a black image on top."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(128, 128, 3), num_classes=21, pre_nms_max_proposals=300,
                          max_proposals=64, max_detections=16)
    d = str(tmp_path)
    weights_mod.save_synthetic_models(d, cfg, seed=4, forced_load=False)
    om = load_oracle_model(d)
    images = rand_images(3, 128, 128, seed=8)
    images[2] = 0                                                        # black frame
    m = models.load_maskrcnn(d, max_batch=3, compute_dtype=mode)
    det, mask = m.predict(images)
    trunk = om.trunk(images)
    counts = []
    for b in range(3):
        d_b, m_b = _check_stages(pkg, orc, om, m, cfg, images, b, True, trunk, f16=(mode == "f16"))
        np.testing.assert_array_equal(det[b], d_b)
        np.testing.assert_array_equal(mask[b].reshape(cfg.max_detections, -1), m_b)
        n = int((d_b[:, 5] > 0).sum())
        counts.append(n)
        assert (d_b[n:] == 0).all() and (m_b[n:] == 0).all()             # zero padding after the last detection
    assert min(counts) < cfg.max_detections, counts                     # the short-count path was taken
    # a second call on other images must not inherit rows from this one
    det2, mask2 = m.predict(images[::-1].copy())
    np.testing.assert_array_equal(det2[::-1], det)
    np.testing.assert_array_equal(mask2[::-1], mask)
    pkg.MaskRCNNConfig.defaultConfig().anchorsURL = None


def test_engine_fp16_range_watchdog(pkg, small_model, weights_mod, tmp_path):
    """Activations beyond the fp16 range: exact in MRCNN_F32; refused (not silently saturated) in MRCNN_F16, whose tensors ARE fp16;
    the split modes — fp32 tensors — RECOVER since round 5 (the batch is measured on the device, the split exponents are lowered, the
    batch is computed again inside the call: "range_recoveries") and agree with the exact-fp32 engine, because the reference's fp32
    path has no such failure (Conversion/task.py:90).  The enqueue-only entry still only reports (check_range)."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    hot = tmp_path / "hot"
    hot.mkdir()
    for kind in ("MaskRCNN", "Classifier", "Mask"):
        meta, tensors = weights_mod.read_mrcw(os.path.join(d, f"{kind}.mrcw"))
        t = dict(tensors)
        if kind == "MaskRCNN":                       # the stem's BatchNorm now multiplies by 2^12: C1 reaches ~1e5
            t["bn_conv1/gamma"] = (t["bn_conv1/gamma"].astype(np.float32) * 4096).astype(np.float16)
        weights_mod.write_mrcw(str(hot / f"{kind}.mrcw"), meta, t)
    __import__("importlib").import_module("mask-rcnn-coreml_amd.anchors").write_anchors_bin(str(hot / "anchors.bin"), cfg)
    images = rand_images(1, cfg.image_height, cfg.image_width, seed=2)
    m32 = models.load_maskrcnn(str(hot), max_batch=1)
    det, _ = m32.predict(images)
    p2 = m32.read_tensor("P2", 0)
    assert np.isfinite(det).all() and m32.get_int("range_overflows") == 0
    m = models.load_maskrcnn(str(hot), max_batch=1, compute_dtype="f16")
    with pytest.raises(Exception, match="left the fp16 range"):
        m.predict(images)
    assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 0
    for mode in ("f32s", "f32x3"):
        m = models.load_maskrcnn(str(hot), max_batch=1, compute_dtype=mode)
        got, _ = m.predict(images)                  # trips, recovers, returns valid records
        assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1
        assert _rel(m.read_tensor("P2", 0), p2) < 5e-5, mode
        assert np.isfinite(got).all()
        m.predict(images)
        assert m.get_int("range_recoveries") == 1   # the lowered exponents hold
    # the same handles are fine on in-range weights
    ok = models.load_maskrcnn(d, max_batch=1, compute_dtype="f32s")
    ok.predict(images)
    assert ok.get_int("range_overflows") == 0
    pkg.MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(d, "anchors.bin")


# ---------------------------------------------------------------------------------------------------------------------
# LOCAL overflows: the first tensor to leave the fp16 range lies past the stem, so Inf / NaN run through the rest of the
# pipeline (ROI align, softmax, the classifier's arg-max, DetectionLayer, the mask select) before the watchdog word is read
# ---------------------------------------------------------------------------------------------------------------------
FP16_LIMIT = 65504.0
TRUNK_TAPS = ["C1", "C2", "C3", "C4", "C5", "P2", "P3", "P4", "P5"]
# (the tap compared after a recovery is the deepest one that is a CONTINUOUS function of the image — a trunk tap or the RPN's deltas: behind the
#  proposal and detection stages two engines that differ by 1e-5 may pick other rows, and no norm compares those; the heads' depths therefore
#  compare P2, as test_engine_fp16_range_watchdog does, and the heads' own tensors only where the discrete stages agreed bit for bit)
LOCAL_OVERFLOWS = {  # depth: (file, convolution, its BatchNorm, the first tensor out of range, taps that must stay in range, tap compared after a recovery,
    #         the next layer whose kernel takes 2^-k so that only the named tensor grows | None: everything behind it grows with it)
    "c5_last_block": ("MaskRCNN", "res5c_branch2c", "bn5c_branch2c", "C5", ["C1", "C2", "C3", "C4"], "C5", None),
    "c5_entry_shortcut": ("MaskRCNN", "res5a_branch1", "bn5a_branch1", "C5", ["C1", "C2", "C3", "C4"], "C5", None),
    "fpn_p3_alone": ("MaskRCNN", "fpn_p3", None, "P3", ["C1", "C2", "C3", "C4", "C5", "P2", "P4", "P5"], "P3", None),
    "rpn_shared_3x3": ("MaskRCNN", "rpn_conv_shared", None, "rpn_feat", TRUNK_TAPS, "rpn_deltas", None),
    "box_head_fc1": ("Classifier", "mrcnn_class_conv1", "mrcnn_class_bn1", "cls_h1", TRUNK_TAPS + ["pooled"], "P2", "mrcnn_class_conv2"),
    "mask_head_conv1": ("Mask", "mrcnn_mask_conv1", "mrcnn_mask_bn1", "mask_t1", TRUNK_TAPS + ["pooled", "pooled_mask"], "P2", "mrcnn_mask_conv2"),
    "box_head_fc1_to_the_logits": ("Classifier", "mrcnn_class_conv1", "mrcnn_class_bn1", "cls_h1", TRUNK_TAPS + ["pooled"], "P2", None),
    "mask_head_conv1_to_the_deconvolution": ("Mask", "mrcnn_mask_conv1", "mrcnn_mask_bn1", "mask_t1", TRUNK_TAPS + ["pooled", "pooled_mask"], "P2", None),
}
# Unrecoverable BY DESIGN in the split modes: behind these edits the heads' last tensors (logits and box deltas; the mask deconvolution's output) grow
# by the same 2^k.  They belong to the FIXED group "outputs" (exponent 0: their consumers are fp32 arithmetic), which a recovery cannot rescale, and
# the epilogues that store them are watched like every other: once they pass 65504 the recomputed batch trips again and the documented error stands.
FIXED_GROUP_DEPTHS = ("box_head_fc1_to_the_logits", "mask_head_conv1_to_the_deconvolution")


def _scaled_layer(tensors, conv, bn, k, comp=None):
    """The layer's output before its activation times 2^k, exactly: kernel, bias (and the BatchNorm mean) carry 2^a, gamma 2^(k-a), beta 2^k —
    every tensor stays fp16-representable (asserted).  comp: the next layer's kernel times 2^-k, rounded to fp16 (its small entries become
    subnormal: the same file feeds every engine compared)."""
    t = dict(tensors)
    if comp:
        t[f"{comp}/kernel"] = np.ldexp(t[f"{comp}/kernel"].astype(np.float32), -k).astype(np.float16)
    a = k // 2 if bn else k
    mul = {f"{conv}/kernel": a, f"{conv}/bias": a}
    if bn:
        mul.update({f"{bn}/mean": a, f"{bn}/gamma": k - a, f"{bn}/beta": k})
    for name, e in mul.items():
        v = np.ldexp(t[name].astype(np.float32), e)
        h = v.astype(np.float16)
        assert np.isfinite(h).all() and np.array_equal(h.astype(np.float32), v), name
        t[name] = h
    return t


def _write_model(weights_mod, src, dst, cfg, edits):
    os.makedirs(dst)
    for kind in ("MaskRCNN", "Classifier", "Mask"):
        meta, tensors = weights_mod.read_mrcw(os.path.join(src, f"{kind}.mrcw"))
        weights_mod.write_mrcw(os.path.join(dst, f"{kind}.mrcw"), meta, edits[kind](tensors) if kind in edits else tensors)
    __import__("importlib").import_module("mask-rcnn-coreml_amd.anchors").write_anchors_bin(os.path.join(dst, "anchors.bin"), cfg)
    return dst


def _bn_fold(tensors, meta, conv, bn):
    f = lambda n: tensors[n].astype(np.float64)
    if not bn:
        return np.ones_like(f(f"{conv}/bias")), f(f"{conv}/bias")
    sc = f(f"{bn}/gamma") / np.sqrt(f(f"{bn}/variance") + float(meta.get("bn_eps", 1e-3)))
    return sc, (f(f"{conv}/bias") - f(f"{bn}/mean")) * sc + f(f"{bn}/beta")


def _first_hot_tensor_absmax(m32, cfg, weights_mod, model_dir, depth, batch):
    """max |v| of the depth's target tensor in the exact-fp32 engine: its tap where it has one; otherwise the layer evaluated in float64 on the
    engine's tap of its INPUT (P2 for the RPN's shared layer — the first level it runs on; the pooled ROI rows for the heads)."""
    import torch
    import torch.nn.functional as F
    kind, conv, bn, target = LOCAL_OVERFLOWS[depth][:4]
    if target in TRUNK_TAPS:
        return max(float(np.abs(m32.read_tensor(target, b)).max()) for b in range(batch))
    meta, tensors = weights_mod.read_mrcw(os.path.join(model_dir, f"{kind}.mrcw"))
    sc, sh = _bn_fold(tensors, meta, conv, bn)
    w = torch.from_numpy(tensors[f"{conv}/kernel"].astype(np.float64))                 # (O, I, kh, kw)
    best = 0.0
    for b in range(batch):
        if target == "rpn_feat":
            h, wd = cfg.feature_shapes()[0]
            x = m32.read_tensor("P2", b).reshape(1, h, wd, 256)
            y = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), w, padding=1)
        elif target == "cls_h1":
            x = m32.read_tensor("pooled", b).reshape(cfg.max_proposals, 7, 7, 256)
            y = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), w)
        else:
            x = m32.read_tensor("pooled_mask", b).reshape(cfg.max_detections, 14, 14, 256)
            y = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), w, padding=1)
        y = torch.relu(y * torch.from_numpy(sc)[None, :, None, None] + torch.from_numpy(sh)[None, :, None, None])
        best = max(best, float(y.abs().max()))
    return best


@pytest.fixture(scope="module")
def local_overflow_models(small_model, weights_mod, tmp_path_factory):
    """depth -> (directory of the edited model, the fp32 engine's tap it is compared on): one weight group times 2^k per depth, k the smallest
    power for which the exact-fp32 engine shows the target tensor beyond TWICE the fp16 range while every tap upstream stays below HALF of it."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    images = rand_images(1, cfg.image_height, cfg.image_width, seed=2)
    base = models.load_maskrcnn(d, max_batch=1)
    base.predict(images)
    root = str(tmp_path_factory.mktemp("local_overflow"))
    out = {}
    for depth, (kind, conv, bn, target, upstream, tap, comp) in LOCAL_OVERFLOWS.items():
        k = int(np.ceil(np.log2(2.2 * FP16_LIMIT / _first_hot_tensor_absmax(base, cfg, weights_mod, d, depth, 1))))
        for attempt in range(4):          # (C5 = relu(2^k branch + shortcut) is not homogeneous in k: one or two more steps may be needed)
            hot = _write_model(weights_mod, d, os.path.join(root, f"{depth}_{k}"), cfg, {kind: lambda t: _scaled_layer(t, conv, bn, k, comp)})
            m32 = models.load_maskrcnn(hot, max_batch=1)
            det32, mask32 = m32.predict(images)
            top = _first_hot_tensor_absmax(m32, cfg, weights_mod, hot, depth, 1)
            if top > 2 * FP16_LIMIT:
                break
            k += 1
        below = {n: float(np.abs(m32.read_tensor(n, 0)).max()) for n in upstream}
        print(f"{depth}: 2^{k}, {target} reaches {top:.4g}, upstream {below}")
        assert top > 2 * FP16_LIMIT, (depth, k, top)
        assert max(below.values()) < FP16_LIMIT / 2, (depth, below)
        assert m32.get_int("range_overflows") == 0
        heads32 = {n: m32.read_tensor(n, 0).copy() for n in ("rois", "cls_bbox", "detections", "pooled_mask")}
        out[depth] = (hot, m32.read_tensor(tap, 0).copy(), det32, heads32)
    __import__("importlib").import_module("mask-rcnn-coreml_amd").MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(d, "anchors.bin")
    return out, images


def cfg_of(model_fixture):
    return model_fixture[1]


def _good_model_still_predicts(models, small_model, images, mode):
    d, cfg = small_model
    ok = models.load_maskrcnn(d, max_batch=1, compute_dtype=mode)
    det, _ = ok.predict(images)
    assert ok.get_int("range_overflows") == 0 and np.isfinite(det).all() and (det[..., 5] > 0).any()


@pytest.mark.parametrize("mode", ["f16", "f32s", "f32x3"])
@pytest.mark.parametrize("depth", list(LOCAL_OVERFLOWS))
def test_engine_local_overflow_is_refused_or_recovered(pkg, small_model, weights_mod, local_overflow_models, depth, mode):
    """One tensor past the stem leaves the fp16 range: MRCNN_F16 refuses the predict, the split modes recompute it with lowered exponents and
    agree with the exact-fp32 engine — at EVERY depth, although everything behind the hot tensor has run on Inf / NaN by the time the word is read.
    Records with range_overflows == 0 are never accepted; no depth may fault; a good model loaded afterwards still predicts."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    table, images = local_overflow_models
    hot, tap32, det32, heads32 = table[depth]
    tap = LOCAL_OVERFLOWS[depth][5]
    m = models.load_maskrcnn(hot, max_batch=1, compute_dtype=mode)
    try:
        if mode == "f16":
            with pytest.raises(Exception, match="left the fp16 range"):
                m.predict(images)
            assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 0
        else:
            if depth in FIXED_GROUP_DEPTHS:              # the documented error after ONE attempted recovery, never records
                with pytest.raises(Exception, match="left the fp16 range"):
                    m.predict(images)
                assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1
            else:
                got, gmask = m.predict(images)           # trips, recovers, returns valid records
                assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1
                assert _rel(m.read_tensor(tap, 0), tap32) < 5e-5, (depth, mode)
                assert np.isfinite(got).all() and np.isfinite(gmask).all()
                # The recomputed HEAD itself, against float64 on this engine's OWN tap of the head's input (two engines' proposals and detections
                # differ in their last bits, so the fp32 engine's head tensors are no reference): the same 5e-5 bar on the box deltas; on the
                # masks the bar applied to the selected class's logits and carried through the sigmoid, whose slope is at most 1/4.
                cfg = cfg_of(small_model)
                if LOCAL_OVERFLOWS[depth][0] == "Classifier":
                    want = _box_head_deltas64(m.read_tensor("pooled", 0), weights_mod, hot, cfg)
                    assert _rel(m.read_tensor("cls_bbox", 0).reshape(want.shape), want) < 5e-5, (depth, mode)
                if LOCAL_OVERFLOWS[depth][0] == "Mask":
                    # (rows in front of the first one the removeZeros rule drops — a pooled row holding an exact zero — keep compact index = row)
                    flags = np.asarray(m.read_tensor("mask_row_flags", 0)).reshape(-1)[:cfg.max_detections]
                    n = int(np.argmin(flags != 0)) if (flags == 0).any() else cfg.max_detections
                    assert n >= 1 and (got[0][:n, 5] > 0).all()
                    logits = _mask_head_maxima(m, weights_mod, hot, cfg, logits_of=got[0][:, 4].astype(np.int64))[:n]
                    want = 1.0 / (1.0 + np.exp(-logits))
                    assert np.abs(gmask[0].reshape(cfg.max_detections, -1)[:n] - want).max() <= 0.25 * 5e-5 * np.abs(logits).max() + 1e-6, (depth, mode)
                m.predict(images)
                assert m.get_int("range_recoveries") == 1   # the lowered exponents hold
    finally:
        pkg.MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(small_model[0], "anchors.bin")
    _good_model_still_predicts(models, small_model, images, mode)


FUSED_FORM_CASES = [  # knob, values, depth (None: the stem's BatchNorm times 2^12, as test_engine_fp16_range_watchdog), modes
    ("conv_stem", (0, 1, 2), None, ("f16", "f32s", "f32x3"), 1),
    ("mask_fused", (0, 1), "mask_head_conv1", ("f16", "f32s", "f32x3"), 1),
    ("mask_fused", (0, 1), "mask_head_conv1_to_the_deconvolution", ("f16",), 1),
]


@pytest.mark.parametrize("knob,values,depth,modes,default", FUSED_FORM_CASES, ids=[c[0] + ("" if c[2] in (None, "mask_head_conv1") else "-" + c[2]) for c in FUSED_FORM_CASES])
def test_engine_overflow_in_the_engine_only_fused_forms(pkg, small_model, weights_mod, local_overflow_models, tmp_path, knob, values, depth, modes, default):
    """The fused stem (kernels_conv_stem.hip) and both forms of the mask head's tail report the same as the launches they replace (the forms that
    need larger levels — fused shortcut, fused RPN heads, the selected-class epilogue as the FIRST site — have tests of their own below)."""
    L = __import__("importlib").import_module("mask-rcnn-coreml_amd._lib")
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    table, images = local_overflow_models
    if depth is None:
        scale = lambda t: {**t, "bn_conv1/gamma": (t["bn_conv1/gamma"].astype(np.float32) * 4096).astype(np.float16)}
        hot = _write_model(weights_mod, d, str(tmp_path / "hot_stem"), cfg, {"MaskRCNN": scale})
    else:
        hot = table[depth][0]
    try:
        for v in values:
            L.check(L.lib().mrcnn_debug_set(knob.encode(), v))
            for mode in modes:
                m = models.load_maskrcnn(hot, max_batch=1, compute_dtype=mode)
                if mode == "f16":
                    with pytest.raises(Exception, match="left the fp16 range"):
                        m.predict(images)
                    assert m.get_int("range_overflows") == 1, (knob, v)
                else:
                    got, _ = m.predict(images)
                    assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1, (knob, v, mode)
                    assert np.isfinite(got).all()
    finally:
        L.check(L.lib().mrcnn_debug_set(knob.encode(), default))
        pkg.MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(d, "anchors.bin")
    _good_model_still_predicts(models, small_model, images, "f16")


def _launch_shapes(m, images):
    """{(M, N, K): launches} and the total of one profiled predict"""
    m.conv_profile_enable(True)
    m.predict(images)
    m.conv_profile_enable(False)
    shapes = {}
    for (M, N, K, tile, n, *_) in m.conv_profile_shapes():
        shapes[(M, N, K)] = shapes.get((M, N, K), 0) + n
    return shapes, sum(shapes.values())


@pytest.mark.parametrize("mode", ["f32s", "f32x3"])
def test_engine_overflow_inside_the_fused_shortcut_launch(pkg, weights_mod, tmp_path_factory, tmp_path, mode):
    """The shortcut computed INSIDE branch2c's launch (conv_device.h: conv_epilogue_wave with the second accumulator set) is a stored tensor of the
    two-launch form, watched there by its own launch; the fused launch must report it as well.  A 320 x 448 model at batch 3, where C2's entry fuses
    (210 M tiles x 2 column tiles; asserted on the launch counts).  bn2a_branch1 gets mean 60000 and four times its gamma: EVERY shortcut value lies
    below -2 x 65504 (float64 on the fp32 engine's C1 tap), so res2a's output is relu(branch + shortcut) = 0 and nothing else in the network
    leaves the range — the shortcut's check is the only site that can trip."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "scfuse_hot" + mode, architecture="resnet50", input_image_shape=(320, 448, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 3
    images = rand_images(B, 320, 448, seed=11)

    def edit(t):
        t = dict(t)
        t["bn2a_branch1/mean"] = np.full_like(t["bn2a_branch1/mean"], 60000.0)
        t["bn2a_branch1/gamma"] = (t["bn2a_branch1/gamma"].astype(np.float32) * 4).astype(np.float16)
        return t
    hot = _write_model(weights_mod, d, str(tmp_path / "hot"), cfg, {"MaskRCNN": edit})
    try:
        m32 = models.load_maskrcnn(hot, max_batch=B)
        det32, _ = m32.predict(images)
        meta, tensors = weights_mod.read_mrcw(os.path.join(hot, "MaskRCNN.mrcw"))
        sc, sh = _bn_fold(tensors, meta, "res2a_branch1", "bn2a_branch1")
        kern = tensors["res2a_branch1/kernel"].astype(np.float64).reshape(256, 64)
        for b in range(B):
            short = m32.read_tensor("C1", b).reshape(-1, 64).astype(np.float64) @ kern.T * sc + sh
            assert short.max() < -2 * FP16_LIMIT, short.max()
            assert max(float(np.abs(m32.read_tensor(n, b)).max()) for n in TRUNK_TAPS) < FP16_LIMIT / 2
        assert m32.get_int("range_overflows") == 0 and np.isfinite(det32).all()
        p2 = m32.read_tensor("P2", 1).copy()
        c2_shape = (B * 80 * 112, 256, 64)          # res2a_branch2c, res2a_branch1 and the branch2c of res2b / res2c
        counts = {}
        for knob in (1, 0):
            L.check(L.lib().mrcnn_debug_set(b"conv_scfuse", knob))
            counts[knob] = _launch_shapes(models.load_maskrcnn(d, max_batch=B, compute_dtype=mode), images)
            m = models.load_maskrcnn(hot, max_batch=B, compute_dtype=mode)
            got, gmask = m.predict(images)
            assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1, (knob, mode)
            assert np.isfinite(got).all() and np.isfinite(gmask).all()
            assert _rel(m.read_tensor("P2", 1), p2) < 5e-5, (knob, mode)
        # the fused form ran at C2 with the knob on: its shortcut is no launch of its own
        assert counts[1][0].get(c2_shape, 0) == 3 and counts[0][0].get(c2_shape, 0) == 4, (counts[1][0].get(c2_shape), counts[0][0].get(c2_shape))
        assert counts[1][1] < counts[0][1]
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_scfuse", 1))
        pkg.MaskRCNNConfig.defaultConfig().anchorsURL = None


@pytest.mark.parametrize("mode", ["f16", "f32s", "f32x3"])
def test_engine_overflow_under_the_fused_rpn_heads(pkg, weights_mod, tmp_path_factory, tmp_path, mode):
    """The RPN's shared 3x3 layer with the two heads in its epilogue (split modes: kernels_conv_halo.hip, HEAD; fp16: kernels_conv3x3_h.hip, HEAD)
    never stores the 512-channel tensor it watches.  A 512^2 model: P2 is 128 x 128 = 16384 pixels, fused in every mode (asserted on the launch
    counts).  rpn_conv_shared times 2^k: the fp32 engine's taps stay below half the range, the shared layer's output on P2 (float64 on a 34 x 34
    crop of the P2 tap: its 32 x 32 interior) passes twice the range.  Fused and unfused forms report the same."""
    import importlib
    import torch
    import torch.nn.functional as F
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "rpnhot" + mode, architecture="resnet50", input_image_shape=(512, 512, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 2
    images = rand_images(B, 512, 512, seed=5)

    def shared_layer_max(m32, model_dir):
        meta, tensors = weights_mod.read_mrcw(os.path.join(model_dir, "MaskRCNN.mrcw"))
        w = torch.from_numpy(tensors["rpn_conv_shared/kernel"].astype(np.float64))
        bias = torch.from_numpy(tensors["rpn_conv_shared/bias"].astype(np.float64))
        x = m32.read_tensor("P2", 0).reshape(128, 128, 256)[:34, :34].astype(np.float64)
        y = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], w) + bias[None, :, None, None]
        return float(torch.relu(y).max())
    knob_name, on, offs = ("conv_c3h", 1, (3, 0)) if mode == "f16" else ("conv_halo", 1, (0,))
    try:
        base = models.load_maskrcnn(d, max_batch=B)
        base.predict(images)
        k = int(np.ceil(np.log2(2.2 * FP16_LIMIT / shared_layer_max(base, d))))
        hot = _write_model(weights_mod, d, str(tmp_path / "hot"), cfg, {"MaskRCNN": lambda t: _scaled_layer(t, "rpn_conv_shared", None, k)})
        m32 = models.load_maskrcnn(hot, max_batch=B)
        m32.predict(images)
        assert shared_layer_max(m32, hot) > 2 * FP16_LIMIT
        for b in range(B):
            assert max(float(np.abs(m32.read_tensor(n, b)).max()) for n in TRUNK_TAPS) < FP16_LIMIT / 2
        deltas32 = m32.read_tensor("rpn_deltas", 0).copy()
        totals = {}
        for v in (on,) + offs:
            L.check(L.lib().mrcnn_debug_set(knob_name.encode(), v))
            totals[v] = _launch_shapes(models.load_maskrcnn(d, max_batch=B, compute_dtype=mode), images)[1]
            m = models.load_maskrcnn(hot, max_batch=B, compute_dtype=mode)
            if mode == "f16":
                with pytest.raises(Exception, match="left the fp16 range"):
                    m.predict(images)
                assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 0, (knob_name, v)
            else:
                got, gmask = m.predict(images)
                assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == 1, (knob_name, v)
                assert np.isfinite(got).all() and np.isfinite(gmask).all()
                assert _rel(m.read_tensor("rpn_deltas", 0), deltas32) < 5e-5, (knob_name, v)
        # with the knob on, fused levels have no head launch of their own
        assert all(totals[on] < totals[v] for v in offs), totals
    finally:
        L.check(L.lib().mrcnn_debug_set(knob_name.encode(), 1))
        pkg.MaskRCNNConfig.defaultConfig().anchorsURL = None


def _box_head_deltas64(pooled, weights_mod, model_dir, cfg):
    """the box head's deltas (rows, nc * 4) in float64 from an engine's pooled tap (rows of 7 x 7 x 256, NHWC)"""
    meta, t = weights_mod.read_mrcw(os.path.join(model_dir, "Classifier.mrcw"))
    x = pooled.reshape(cfg.max_proposals, -1).astype(np.float64)
    for conv, bn in (("mrcnn_class_conv1", "mrcnn_class_bn1"), ("mrcnn_class_conv2", "mrcnn_class_bn2")):
        k = t[f"{conv}/kernel"].astype(np.float64)
        sc, sh = _bn_fold(t, meta, conv, bn)
        x = np.maximum(x @ k.transpose(0, 2, 3, 1).reshape(k.shape[0], -1).T * sc + sh, 0.0)
    return x @ t["mrcnn_bbox_fc/kernel"].astype(np.float64).T + t["mrcnn_bbox_fc/bias"].astype(np.float64)


def _mask_head_maxima(m32, weights_mod, model_dir, cfg, logits_of=None):
    """max |v| of the mask head's five stored tensors (four 3x3 layers, the deconvolution) in float64 on an engine's pooled_mask tap;
    logits_of = class ids per row: instead, the (rows, 28 * 28) logits of those classes"""
    import torch
    import torch.nn.functional as F
    meta, t = weights_mod.read_mrcw(os.path.join(model_dir, "Mask.mrcw"))
    x = torch.from_numpy(m32.read_tensor("pooled_mask", 0).reshape(cfg.max_detections, 14, 14, 256).astype(np.float64)).permute(0, 3, 1, 2)
    out = []
    for i in range(1, 5):
        sc, sh = _bn_fold(t, meta, f"mrcnn_mask_conv{i}", f"mrcnn_mask_bn{i}")
        x = F.conv2d(x, torch.from_numpy(t[f"mrcnn_mask_conv{i}/kernel"].astype(np.float64)), padding=1)
        x = torch.relu(x * torch.from_numpy(sc)[None, :, None, None] + torch.from_numpy(sh)[None, :, None, None])
        out.append(float(x.abs().max()))
    y = F.conv_transpose2d(x, torch.from_numpy(t["mrcnn_mask_deconv/kernel"].astype(np.float64)), stride=2)
    y = torch.relu(y + torch.from_numpy(t["mrcnn_mask_deconv/bias"].astype(np.float64))[None, :, None, None])
    if logits_of is not None:
        z = F.conv2d(y, torch.from_numpy(t["mrcnn_mask/kernel"].astype(np.float64))) + torch.from_numpy(t["mrcnn_mask/bias"].astype(np.float64))[None, :, None, None]
        return z.numpy()[np.arange(z.shape[0]), logits_of].reshape(z.shape[0], -1)
    return out + [float(y.abs().max())]


@pytest.mark.parametrize("mode", ["f16", "f32s", "f32x3"])
def test_engine_overflow_first_in_the_mask_deconvolution(pkg, small_model, weights_mod, tmp_path, mode):
    """The mask head's last stored tensor: with "mask_fused" 1 it exists only inside the deconvolution's selected-class epilogue
    (conv_device.h: conv_epilogue_sel_wave), which therefore carries the watch; with 0 the tensor is stored and selected from.  mrcnn_mask_deconv
    times 2^k: the four layers in front stay below half the range, the deconvolution's output passes twice the range (float64 on the fp32 engine's
    pooled_mask tap).  It belongs to the fixed group `outputs` (FIXED_GROUP_DEPTHS): fp16 refuses, the split modes end in the documented error after
    one attempted recovery — the same with either form."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    images = rand_images(1, cfg.image_height, cfg.image_width, seed=2)
    try:
        base = models.load_maskrcnn(d, max_batch=1)
        base.predict(images)
        k = int(np.ceil(np.log2(2.2 * FP16_LIMIT / _mask_head_maxima(base, weights_mod, d, cfg)[4])))
        hot = _write_model(weights_mod, d, str(tmp_path / "hot"), cfg, {"Mask": lambda t: _scaled_layer(t, "mrcnn_mask_deconv", None, k)})
        m32 = models.load_maskrcnn(hot, max_batch=1)
        det32, mask32 = m32.predict(images)
        mx = _mask_head_maxima(m32, weights_mod, hot, cfg)
        assert max(mx[:4]) < FP16_LIMIT / 2 and mx[4] > 2 * FP16_LIMIT, mx
        assert max(float(np.abs(m32.read_tensor(n, 0)).max()) for n in TRUNK_TAPS + ["pooled", "pooled_mask"]) < FP16_LIMIT / 2
        assert np.isfinite(det32).all() and np.isfinite(mask32).all() and m32.get_int("range_overflows") == 0
        for fused in (1, 0):
            L.check(L.lib().mrcnn_debug_set(b"mask_fused", fused))
            m = models.load_maskrcnn(hot, max_batch=1, compute_dtype=mode)
            with pytest.raises(Exception, match="left the fp16 range"):
                m.predict(images)
            assert m.get_int("range_overflows") == 1 and m.get_int("range_recoveries") == (0 if mode == "f16" else 1), (fused, mode)
    finally:
        L.check(L.lib().mrcnn_debug_set(b"mask_fused", 1))
        pkg.MaskRCNNConfig.defaultConfig().anchorsURL = os.path.join(d, "anchors.bin")
    _good_model_still_predicts(models, small_model, images, mode)


@pytest.mark.parametrize("mode", ["f32s", "f32x3"])
def test_engine_f32s_full_size(pkg, orc, tmp_path_factory, weights_mod, mode):
    """BASELINE configs[1] shapes (R101, 1024², 81 classes) in the split modes, batch 2: staged parity at fp32 tolerances."""
    from oracle.network import load_oracle_model
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "full" + mode, architecture="resnet101")
    om = load_oracle_model(d)
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype=mode)
    images = rand_images(2, 1024, 1024, seed=1)
    m.predict(images)
    trunk = om.trunk(images[:1])
    d0, _ = _check_stages(pkg, orc, om, m, cfg, images, 0, True, trunk)
    _check_stages(pkg, orc, om, m, cfg, images, 1, False)
    assert int(m.read_tensor("keep_count", 0)[0]) == cfg.max_proposals
    assert int((d0[:, 5] > 0).sum()) == cfg.max_detections


def test_engine_lifecycle_streams_and_handles(pkg, small_model):
    """Handles are independent and leak-free: load/destroy cycles give the HBM back, two live handles do not
    disturb each other, and a handle moved onto the caller's stream (mrcnn_model_set_stream + predict_async,
    the torch-interop path of bench.py) gives the results of the synchronous call."""
    import gc
    import torch
    il = __import__("importlib")
    models, L = il.import_module("mask-rcnn-coreml_amd.models"), il.import_module("mask-rcnn-coreml_amd._lib")
    d, cfg = small_model
    images = rand_images(3, cfg.image_height, cfg.image_width, seed=13)
    m1 = models.load_maskrcnn(d, max_batch=3)
    det_ref, mask_ref = m1.predict(images)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        m = models.load_maskrcnn(d, max_batch=3)
        det, mask = m.predict(images)
        np.testing.assert_array_equal(det, det_ref)
        del m
        gc.collect()
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) < 32 << 20, "model handles leak device memory"
    L.lib().mrcnn_model_destroy(None)                        # NULL is a no-op, like free()

    # two live handles with different arenas, interleaved calls
    m2 = models.load_maskrcnn(d, max_batch=1)
    for b in range(3):
        d2, k2 = m2.predict(images[b:b + 1])
        d1, k1 = m1.predict(images[::-1].copy())
        np.testing.assert_array_equal(d2[0], det_ref[b])
        np.testing.assert_array_equal(k2[0], mask_ref[b])
        np.testing.assert_array_equal(d1[::-1], det_ref)

    # the caller's stream: enqueue-only predict ordered after work the caller queued on that stream
    st = torch.cuda.Stream()
    m1.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        img_d = torch.from_numpy(images).cuda(non_blocking=True)     # H2D queued on st, predict must see it
        det_d = torch.full((3, m1.max_detections, 6), float("nan"), device="cuda")
        mask_d = torch.full((3, m1.max_detections, m1.mask_size, m1.mask_size), float("nan"), device="cuda")
        m1.predict_into(img_d, det_d, mask_d, sync=False)
        total = det_d[:, :, 5].sum()                                 # consumer queued behind predict on st
    st.synchronize()
    np.testing.assert_array_equal(det_d.cpu().numpy(), det_ref)
    np.testing.assert_array_equal(mask_d.cpu().numpy(), mask_ref)
    assert float(total) == float(det_ref[:, :, 5].astype(np.float32).sum(dtype=np.float32)) or abs(float(total) - det_ref[:, :, 5].sum()) < 1e-3


@pytest.mark.parametrize("mode", ["f32", "f32x3", "f16"])
def test_fused_mask_tail_equals_deconvolution_plus_select(pkg, weights_mod, tmp_path_factory, mode):
    """The mask head's tail as shipped (the deconvolution's epilogue takes the dot with the selected class's 1x1 filter and a
    small kernel adds the two 128-channel partials) against the unfused form (256-channel deconvolution output + k_mask_select):
    same detections, same set of written / zero rows, masks within the fp32 summation-order noise of a 256-term dot."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    L = __import__("importlib").import_module("mask-rcnn-coreml_amd._lib")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(256, 256, 3), num_classes=7, max_detections=20)
    d = str(tmp_path_factory.mktemp("fuse_" + mode))
    weights_mod.save_synthetic_models(d, cfg, seed=5, forced_load=True)
    m = models.load_maskrcnn(d, max_batch=3, compute_dtype=mode)
    imgs = np.random.default_rng(9).integers(0, 256, (3, 256, 256, 3), dtype=np.uint8)
    try:
        L.check(L.lib().mrcnn_debug_set(b"mask_fused", 0))
        d0, k0 = m.predict(imgs)
        L.check(L.lib().mrcnn_debug_set(b"mask_fused", 1))
        d1, k1 = m.predict(imgs)
    finally:
        L.check(L.lib().mrcnn_debug_set(b"mask_fused", 1))
    np.testing.assert_array_equal(d1, d0)
    np.testing.assert_array_equal((k1 == 0).all(axis=(2, 3)), (k0 == 0).all(axis=(2, 3)))
    assert (d0[..., 5] > 0).sum() > 0 and np.abs(k1 - k0).max() < 2e-6


def test_engine_graph_replay_matches_stream_launches(pkg, small_model):
    """Opt-in hipGraph replay: captured on the second call per batch size, identical results, bypassed (not broken)
    while the profilers record events, and droppable."""
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=2)
    assert m.get_int("graph_enabled") == 0
    imgs = [rand_images(b, cfg.image_height, cfg.image_width, seed=30 + b) for b in (1, 2)]
    ref = [m.predict(i) for i in imgs]
    m.enable_graph(True)
    for rep in range(3):                                  # eager, capture + launch, launch
        for i, r in zip(imgs, ref):
            det, mask = m.predict(i)
            np.testing.assert_array_equal(det, r[0])
            np.testing.assert_array_equal(mask, r[1])
    assert m.get_int("graph_launches") == 4               # 2 batch sizes × (rep 1, rep 2)
    m.enable_timing(True)                                 # events between launches: replay is bypassed
    det, _ = m.predict(imgs[1])
    np.testing.assert_array_equal(det, ref[1][0])
    assert m.get_int("graph_launches") == 4 and m.stage_ms()["Trunk"] > 0
    m.enable_timing(False)
    m.predict(imgs[1])
    assert m.get_int("graph_launches") == 5
    m.enable_graph(False)
    det, mask = m.predict(imgs[0])
    np.testing.assert_array_equal(det, ref[0][0])
    assert m.get_int("graph_launches") == 5 and m.get_int("graph_enabled") == 0


def test_engine_joins_a_callers_graph_capture(pkg, small_model):
    """A caller that captures its own stream (here: torch.cuda.graph) gets predict_async's launches recorded into ITS graph:
    replaying that graph on new input reproduces the eager results."""
    import torch
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=2)
    imgs_a = rand_images(2, cfg.image_height, cfg.image_width, seed=41)
    imgs_b = rand_images(2, cfg.image_height, cfg.image_width, seed=42)
    ref_a, ref_b = m.predict(imgs_a), m.predict(imgs_b)           # also the one-time host set-up, outside any capture
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    img_d = torch.from_numpy(imgs_a).cuda()
    det_d = torch.zeros((2, m.max_detections, 6), device="cuda")
    mask_d = torch.zeros((2, m.max_detections, m.mask_size, m.mask_size), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        m.predict_into(img_d, det_d, mask_d, sync=False)
    det_d.zero_(); mask_d.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(det_d.cpu().numpy(), ref_a[0])
    np.testing.assert_array_equal(mask_d.cpu().numpy(), ref_a[1])
    img_d.copy_(torch.from_numpy(imgs_b).cuda())
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(det_d.cpu().numpy(), ref_b[0])
    np.testing.assert_array_equal(mask_d.cpu().numpy(), ref_b[1])


@pytest.mark.parametrize("mode", ["f32x3", "f16"])
def test_predict_scalefit_equals_letterbox_then_predict(pkg, small_model, mode):
    """mrcnn_maskrcnn_predict_scalefit (`.scaleFit` of EvaluateCommand.swift:152-157 inside predict): images of
    any size — landscape, portrait, smaller and larger than the model, and exactly the model's size — give bit for bit what
    mrcnn_letterbox_rgb followed by mrcnn_maskrcnn_predict gives; mrcnn_unletterbox_boxes equals the Python mirror."""
    import ctypes as C
    models = __import__("importlib").import_module("mask-rcnn-coreml_amd.models")
    ev = __import__("importlib").import_module("mask-rcnn-coreml_amd.evaluate")
    L = __import__("importlib").import_module("mask-rcnn-coreml_amd._lib")
    d, cfg = small_model
    H, W = cfg.image_height, cfg.image_width
    m = models.load_maskrcnn(d, max_batch=3, compute_dtype=mode)
    rng = np.random.default_rng(41)
    for (h, w, B) in ((96, 160, 2), (300, 200, 3), (H, W, 1), (37, 53, 2)):
        imgs = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
        det, mask = m.predict_scalefit(imgs)
        boxed = np.stack([ev.letterbox(imgs[b], H, W) for b in range(B)])
        if (h, w) == (H, W):
            np.testing.assert_array_equal(boxed, imgs)                  # the identity case really is the identity
        det0, mask0 = m.predict(boxed)
        np.testing.assert_array_equal(det, det0)
        np.testing.assert_array_equal(mask, mask0)
        un = det[0].copy()
        L.check(L.lib().mrcnn_unletterbox_boxes(un.ctypes.data, un.shape[0], 6, h, w, H, W))
        np.testing.assert_allclose(un[:, :4], ev.unletterbox_boxes(det[0], h, w, H, W)[:, :4].astype(np.float32), rtol=0, atol=1e-7)
        np.testing.assert_array_equal(un[:, 4:], det[0][:, 4:])
    # a plain predict in between sees no state of the scale-fit path
    img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    d1, k1 = m.predict(img)
    d2, k2 = m.predict_scalefit(img)
    np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(k1, k2)
    with pytest.raises(L.MrcnnError):
        m.predict(rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8))      # the exact-size entry still refuses other sizes
    pkg.MaskRCNNConfig.defaultConfig().anchorsURL = None


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_halo_tile_geometry_leaves_predict_bit_identical(pkg, weights_mod, tmp_path_factory, dtype):
    """Round 4: the halo kernel's tiles at P2 / P3 of a 512² input are two rows x 64 columns (round 3: one row x 128), incl. the
    instantiation that carries the fused RPN heads; which pixels a tile owns must not change one bit of a predict
    (mrcnn_debug_set("halo_geo", 0) = the round-3 geometries)."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "geo512", architecture="resnet50", input_image_shape=(512, 512, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 2
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype=dtype)
    images = rand_images(B, 512, 512, seed=5)
    det, mask = m.predict(images)
    taps = {n: [m.read_tensor(n, b).copy() for b in range(B)] for n in ("rpn_probs", "rpn_deltas", "P2", "P3", "P4", "P5")}
    try:
        L.check(L.lib().mrcnn_debug_set(b"halo_geo", 0))
        det3, mask3 = m.predict(images)
        for n, want in taps.items():
            for b in range(B):
                np.testing.assert_array_equal(m.read_tensor(n, b), want[b], err_msg=f"{n} image {b}")
    finally:
        L.check(L.lib().mrcnn_debug_set(b"halo_geo", 1))
    np.testing.assert_array_equal(det, det3)
    np.testing.assert_array_equal(mask, mask3)
    assert (det[..., 5] > 0).sum() > 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s", "f16"])
def test_fused_stem_is_bit_identical_to_conv1_plus_maxpool(pkg, weights_mod, tmp_path_factory, dtype):
    """Round 4: in the split modes and in fp16 mode conv1 (7x7 / 2 + BatchNorm + ReLU) and the 3x3 / 2 max-pool run as ONE persistent launch
    (kernels_conv_stem.hip: the input patch of a 3 x 16 block of pooled outputs is loaded and split once; conv1's output never
    exists) with the 128-row kernel's arithmetic in its K order: a predict must not change by one bit against the two launches
    (mrcnn_debug_set("conv_stem", 0)) — odd image sizes in tiles (a 320 x 448 input: ragged last tile row, right / bottom pool
    clipping), several images, and per-image results independent of the batch."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "stem" + dtype, architecture="resnet50", input_image_shape=(320, 448, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 3
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype=dtype)
    images = rand_images(B, 320, 448, seed=9)
    det, mask = m.predict(images)
    taps = {n: [m.read_tensor(n, b).copy() for b in range(B)] for n in ("rpn_probs", "rpn_deltas", "P2", "P5")}
    try:
        if dtype == "f16":
            # round 5: the default fp16 form drops the zero channels of the staged pixels (two K groups per kernel row instead of four): the 16
            # products of an MFMA group differently, so it agrees with the four-group form ("conv_stem" 2) to summation noise — a rare one-ulp
            # flip of an fp16 output — while the four-group form stays bit-identical to the two launches
            L.check(L.lib().mrcnn_debug_set(b"conv_stem", 2))
            det, mask = m.predict(images)
            for n, compact in taps.items():
                for b in range(B):
                    four = m.read_tensor(n, b)
                    # (measured: 2.8e-3 on an RPN probability — one fp16 ulp of a stem output, carried through 50 fp16 layers)
                    assert np.abs(four - compact[b]).max() <= 6e-3 * max(1.0, np.abs(four).max()), n
            taps = {n: [m.read_tensor(n, b).copy() for b in range(B)] for n in taps}
        L.check(L.lib().mrcnn_debug_set(b"conv_stem", 0))
        det2, mask2 = m.predict(images)
        for n, want in taps.items():
            for b in range(B):
                np.testing.assert_array_equal(m.read_tensor(n, b), want[b], err_msg=f"{n} image {b}")
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_stem", 1))
    np.testing.assert_array_equal(det, det2)
    np.testing.assert_array_equal(mask, mask2)
    det, mask = m.predict(images)
    d1, m1 = m.predict(images[2:3])
    np.testing.assert_array_equal(d1[0], det[2])
    assert (det[..., 5] > 0).sum() > 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_fused_shortcut_is_bit_identical_to_the_two_launches(pkg, weights_mod, tmp_path_factory, dtype):
    """Round 4 (late): at the entry of a ResNet stage `branch1` (the shortcut, a 1x1 over the block's input) rides inside the launch of
    `branch2c`, which would have read its output as the residual: the shortcut's K loop first, its sums waiting in the second
    accumulator set, the residual formed in the epilogue with the shortcut's own scale / shift — the shortcut tensor is never written.
    Same fp32 operations: a predict must not change by one bit against mrcnn_debug_set("conv_scfuse", 0) — stride-2 shortcuts (C3..C5),
    ragged tiles (a 320 x 448 input), several images, calibrated exponents, and per-image results independent of the batch."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "scfuse" + dtype, architecture="resnet50", input_image_shape=(320, 448, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 3
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype=dtype)
    images = rand_images(B, 320, 448, seed=11)
    m.calibrate_split(images[:2])
    det, mask = m.predict(images)
    names = ("P2", "P3", "P4", "P5", "rpn_probs", "rpn_deltas")         # every stage's output feeds one of them
    taps = {n: [m.read_tensor(n, b).copy() for b in range(B)] for n in names}
    try:
        L.check(L.lib().mrcnn_debug_set(b"conv_scfuse", 0))
        det2, mask2 = m.predict(images)
        for n, want in taps.items():
            for b in range(B):
                np.testing.assert_array_equal(m.read_tensor(n, b), want[b], err_msg=f"{n} image {b}")
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_scfuse", 1))
    np.testing.assert_array_equal(det, det2)
    np.testing.assert_array_equal(mask, mask2)
    d1, m1 = m.predict(images[2:3])
    np.testing.assert_array_equal(d1[0], det[2])
    assert (det[..., 5] > 0).sum() > 0


@pytest.mark.parametrize("arch,shape", [("resnet50", (320, 448, 3)), ("resnet101", (256, 256, 3))])
def test_fused_bottleneck_blocks_leave_an_fp16_predict_bit_identical(pkg, weights_mod, tmp_path_factory, arch, shape):
    """Round 5: in the fp16 mode every identity block of C2..C4 whose level tiles into TH x 16 pixels runs as ONE persistent launch with
    both branch tensors on chip (kernels_bneck.hip).  Same K orders, same fp16 roundings, same epilogue arithmetic: a predict must not
    change by one bit against mrcnn_debug_set("conv_bneck", 0) (the three launches over the same ping-pong tensors), on several images,
    with stages that qualify (C2 at 80 x 112, C3 at 32 x 32 ...) next to stages that do not (C3 at 40 x 56), and per-image results must
    not depend on the batch."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "bneck" + arch, architecture=arch, input_image_shape=shape,
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 3
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype="f16")
    images = rand_images(B, shape[0], shape[1], seed=5)
    L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 3))          # fused at EVERY grid size (by default an under-filled grid takes the three launches)
    det, mask = m.predict(images)
    names = ("P2", "P3", "P4", "P5", "rpn_probs", "rpn_deltas")
    taps = {n: [m.read_tensor(n, b).copy() for b in range(B)] for n in names}
    L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 1))          # the default policy: same bits
    det1, mask1 = m.predict(images)
    np.testing.assert_array_equal(det, det1)
    np.testing.assert_array_equal(mask, mask1)
    try:
        L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 0))
        det2, mask2 = m.predict(images)
        for n, want in taps.items():
            for b in range(B):
                np.testing.assert_array_equal(m.read_tensor(n, b), want[b], err_msg=f"{n} image {b}")
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 1))
    np.testing.assert_array_equal(det, det2)
    np.testing.assert_array_equal(mask, mask2)
    L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 3))
    try:
        d1, m1 = m.predict(images[2:3])
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_bneck", 1))
    np.testing.assert_array_equal(d1[0], det[2])
    assert np.isfinite(taps["P2"][0]).all()


def test_fp16_fused_rpn_heads_equal_the_separate_head_launches(pkg, weights_mod, tmp_path_factory):
    """Round 5: in the fp16 mode the RPN's class / box heads ride in the epilogue of the shared 3x3 layer on the levels with >= 16384 pixels
    (kernels_conv3x3_h.hip, HEAD): the 512-channel tensor is neither written nor read.  Against the same 3x3 kernel followed by the
    separate head launch ("conv_c3h" 3) the logits and deltas — hence every later stage — must agree BIT FOR BIT; against the older
    kernels of the 3x3 layer ("conv_c3h" 0: another K order) within fp16 summation noise; and images must not depend on the batch."""
    import importlib
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, "rpnhead16", architecture="resnet50", input_image_shape=(1024, 768, 3),
                            num_classes=21, pre_nms_max_proposals=1000, max_proposals=128, max_detections=32)
    B = 2
    m = models.load_maskrcnn(d, max_batch=B, compute_dtype="f16")
    images = rand_images(B, 1024, 768, seed=13)
    det, mask = m.predict(images)                         # default: heads fused where a level has >= 16384 pixels: P2 (256 x 192) here; P3 (128 x 96) and up: separate
    probs = [m.read_tensor("rpn_probs", b).copy() for b in range(B)]
    deltas = [m.read_tensor("rpn_deltas", b).copy() for b in range(B)]
    try:
        L.check(L.lib().mrcnn_debug_set(b"conv_c3h", 3))
        det3, mask3 = m.predict(images)
        for b in range(B):
            np.testing.assert_array_equal(m.read_tensor("rpn_probs", b), probs[b])
            np.testing.assert_array_equal(m.read_tensor("rpn_deltas", b), deltas[b])
        np.testing.assert_array_equal(det3, det)
        np.testing.assert_array_equal(mask3, mask)
        L.check(L.lib().mrcnn_debug_set(b"conv_c3h", 0))
        m.predict(images)
        for b in range(B):
            assert np.abs(m.read_tensor("rpn_probs", b) - probs[b]).max() < 5e-3
            assert np.abs(m.read_tensor("rpn_deltas", b) - deltas[b]).max() < 5e-2 * max(1.0, np.abs(deltas[b]).max())
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_c3h", 1))
    d1, m1 = m.predict(images[1:2])
    np.testing.assert_array_equal(d1[0], det[1])
    assert np.isfinite(probs[0]).all() and (det[..., 5] > 0).sum() > 0
