"""Oracle network: a plain torch-CPU fp32 definition of the graph the reference executes.

TEST INFRASTRUCTURE ONLY (see mrcnn_oracle.c).  PARITY STATUS: parity unpinned — the layer list is
the Matterport Mask R-CNN layout (ResNet-50/101 + FPN + RPN, box head, mask head) defined in the
un-vendored, un-pinned third-party package ``edouardlp/Mask-RCNN-Keras`` that the reference's
converter imports (``Sources/maskrcnn/Python/Conversion/task.py:12-13,171-173``); this repo has no
copy of it, so the topology below is restated from the published Matterport model and declared an
assumption.  Data layout is Core ML's: NCHW activations, OIHW kernels,
fp16-stored weights (task.py:90) computed in fp32 (Core ML CPU path).

The custom layers are executed by oracle/oracle.py (C restatement of the Swift sources).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from oracle import oracle as orc  # noqa: E402

_pkg = importlib.import_module("mask-rcnn-coreml_amd")
weights_mod = importlib.import_module("mask-rcnn-coreml_amd.weights")     # the .mrcw container reader only
BN_EPS = 1e-3       # Keras BatchNormalization epsilon of the published Matterport graph (stated here, not imported)


def _stage_blocks(architecture: str):
    """Residual block letters per stage of the published ResNet-50 / ResNet-101 (stage 4: 6 / 23 blocks) — the oracle's own
    table, so that a wrong layer list in the product cannot be shared by the checker."""
    n4 = {"resnet50": 6, "resnet101": 23}[architecture]
    return {2: ["a", "b", "c"], 3: ["a", "b", "c", "d"], 4: [chr(ord("a") + i) for i in range(n4)], 5: ["a", "b", "c"]}


def _bn_of(conv: str):
    """The BatchNormalization that follows a convolution in the published graph (Keras naming), or None."""
    if conv == "conv1":
        return "bn_conv1"
    if conv.startswith("res"):
        return "bn" + conv[3:]
    for head in ("mrcnn_class_", "mrcnn_mask_"):
        if conv.startswith(head + "conv"):
            return head + "bn" + conv[len(head) + 4:]
    return None


def fold_bn_f32(tensors, conv: str, eps: float = BN_EPS):
    """(scale, shift) of conv(+bias)(+BN) as the engine folds them (csrc/engine_weights.hip fold_bn): float32 arithmetic,
    y = acc * scale + shift with scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta."""
    f32 = lambda k: np.asarray(tensors[k], dtype=np.float32)
    bias = f32(f"{conv}/bias")
    bn = _bn_of(conv)
    if bn is None or f"{bn}/gamma" not in tensors:
        return np.ones_like(bias), bias.copy()
    sc = f32(f"{bn}/gamma") / np.sqrt(f32(f"{bn}/variance") + np.float32(eps))
    return sc.astype(np.float32), ((bias - f32(f"{bn}/mean")) * sc + f32(f"{bn}/beta")).astype(np.float32)


class _W:
    """folded=True (float64 evaluations): conv() applies the whole float32-folded affine of conv + BN (fold_bn_f32) and bn() is the
    identity, so that a float64 evaluation measures the convolution arithmetic only, not the fold's rounding."""

    def __init__(self, tensors, dtype=torch.float32, folded=False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32).copy()).to(dtype) for k, v in tensors.items()}
        self.folded = folded
        self.aff = {}
        if folded:
            for k in tensors:
                if k.endswith("/kernel") and f"{k[:-7]}/bias" in tensors:
                    sc, sh = fold_bn_f32(tensors, k[:-7])
                    self.aff[k[:-7]] = (torch.from_numpy(sc).to(dtype), torch.from_numpy(sh).to(dtype))

    def affine(self, y, name):
        sc, sh = self.aff[name]
        shape = (1, -1) + (1,) * (y.dim() - 2)
        return y * sc.reshape(shape) + sh.reshape(shape)

    def conv(self, x, name, stride=1, padding=0):
        if self.folded:
            return self.affine(F.conv2d(x, self.t[f"{name}/kernel"], None, stride=stride, padding=padding), name)
        return F.conv2d(x, self.t[f"{name}/kernel"], self.t[f"{name}/bias"], stride=stride, padding=padding)

    def bn(self, x, name):
        if self.folded:
            return x
        return F.batch_norm(x, self.t[f"{name}/mean"], self.t[f"{name}/variance"], self.t[f"{name}/gamma"],
                            self.t[f"{name}/beta"], training=False, eps=BN_EPS)


def round_to_f16(x):
    """Rounds a float64 tensor (torch or numpy) to fp16 and widens it back: the store of an fp16 activation tensor."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float16).to(torch.float64)
    return np.asarray(x).astype(np.float16).astype(np.float64)


def _same(x):
    return x


def channel_error(x, ref, axis=1, floor=1e-2):
    """max over channels c of max |x - ref|_c / max(max |ref|_c, floor * max |ref|): an error in a small-magnitude channel does not
    hide behind the tensor's maximum; a channel whose whole range lies below `floor` of the tensor's is measured at that scale."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    x = x.reshape(-1, x.shape[-1])
    ref = np.moveaxis(np.asarray(ref, np.float64), axis, -1).reshape(x.shape)
    den = np.maximum(np.abs(ref).max(axis=0), floor * max(float(np.abs(ref).max()), 1e-300))
    return float((np.abs(x - ref).max(axis=0) / den).max())


class OracleMaskRCNN:
    """MaskRCNN.mlmodel + Classifier.mlmodel + Mask.mlmodel + the five custom layers, on CPU."""

    def __init__(self, cfg, main_tensors, classifier_tensors, mask_tensors, anchors):
        self.cfg = cfg
        self.w = _W(main_tensors)
        self.wc = _W(classifier_tensors)
        self.wm = _W(mask_tensors)
        self.anchors = np.ascontiguousarray(anchors, dtype=np.float32)

    # ---- MaskRCNN.mlmodel built-in layers ------------------------------------------------------
    def preprocess(self, images_u8):
        """images (B,H,W,3) uint8 RGB → (B,3,H,W) fp32 minus per-channel mean (task.py:73-75)."""
        x = torch.from_numpy(np.ascontiguousarray(images_u8)).to(torch.float32)
        mean = torch.tensor(self.cfg.mean_rgb, dtype=torch.float32)
        return (x - mean).permute(0, 3, 1, 2).contiguous()

    def _block(self, x, stage, block, stride, has_shortcut):
        w = self.w
        p = f"{stage}{block}"
        y = F.relu(w.bn(w.conv(x, f"res{p}_branch2a", stride=stride), f"bn{p}_branch2a"))
        y = F.relu(w.bn(w.conv(y, f"res{p}_branch2b", padding=1), f"bn{p}_branch2b"))
        y = w.bn(w.conv(y, f"res{p}_branch2c"), f"bn{p}_branch2c")
        sc = w.bn(w.conv(x, f"res{p}_branch1", stride=stride), f"bn{p}_branch1") if has_shortcut else x
        return F.relu(y + sc)

    def backbone(self, x):
        w = self.w
        x = F.pad(x, (3, 3, 3, 3))
        x = F.relu(w.bn(w.conv(x, "conv1", stride=2), "bn_conv1"))
        x = F.pad(x, (0, 1, 0, 1), value=float("-inf"))          # Keras 'same' pool: pad bottom/right
        x = F.max_pool2d(x, 3, 2)
        blocks = _stage_blocks(self.cfg.architecture)
        feats = []
        for stage in (2, 3, 4, 5):
            for b in blocks[stage]:
                first = b == "a"
                x = self._block(x, stage, b, 2 if (first and stage > 2) else 1, first)
            feats.append(x)
        return feats                                              # C2..C5

    def fpn(self, feats):
        w = self.w
        c2, c3, c4, c5 = feats
        p5 = w.conv(c5, "fpn_c5p5")
        p4 = F.interpolate(p5, scale_factor=2, mode="nearest") + w.conv(c4, "fpn_c4p4")
        p3 = F.interpolate(p4, scale_factor=2, mode="nearest") + w.conv(c3, "fpn_c3p3")
        p2 = F.interpolate(p3, scale_factor=2, mode="nearest") + w.conv(c2, "fpn_c2p2")
        p2 = w.conv(p2, "fpn_p2", padding=1)
        p3 = w.conv(p3, "fpn_p3", padding=1)
        p4 = w.conv(p4, "fpn_p4", padding=1)
        p5 = w.conv(p5, "fpn_p5", padding=1)
        p6 = p5[:, :, ::2, ::2]                                   # MaxPool(pool 1, stride 2)
        return [p2, p3, p4, p5, p6]

    def rpn(self, pyramid):
        w = self.w
        probs, deltas = [], []
        for p in pyramid:
            s = F.relu(w.conv(p, "rpn_conv_shared", padding=1))
            lg = w.conv(s, "rpn_class_raw").permute(0, 2, 3, 1)   # (B,H,W,2*na) → (B, H*W*na, 2)
            lg = lg.reshape(lg.shape[0], -1, 2)
            probs.append(F.softmax(lg, dim=-1))
            bb = w.conv(s, "rpn_bbox_pred").permute(0, 2, 3, 1)
            deltas.append(bb.reshape(bb.shape[0], -1, 4))
        return torch.cat(probs, 1), torch.cat(deltas, 1)

    def trunk(self, images_u8):
        with torch.no_grad():
            x = self.preprocess(images_u8)
            pyr = self.fpn(self.backbone(x))
            probs, deltas = self.rpn(pyr)
        return [p.numpy() for p in pyr[:4]], probs.numpy(), deltas.numpy()

    # ---- the same graph in float64, stage by stage ------------------------------------------------
    # Each stage takes its input as given (NCHW, any float dtype; the parity tests hand it the HIP engine's own tap of that input)
    # and evaluates in float64: weights are the artefact's fp16-exact values widened, every conv(+BN) is applied as the float32
    # scale / shift the engine folds (fold_bn_f32), means are the config's float32 values.  What remains between a stage's output
    # and an engine's tap of it is then the engine's convolution arithmetic (summation order, operand split) and its stores.
    #
    # round_f16=True: every tensor the fp16 compute mode STORES is rounded to fp16 where the engine stores it (csrc/engine_plan.hip, csrc/engine_heads.hip):
    #   stem: the mean-subtracted input (the fp16 staging tensor), conv1's output (max-pooled after rounding: max commutes with it);
    #   each bottleneck: branch2a's and branch2b's outputs, the first block's shortcut (branch1) output, the block output;
    #   FPN: the lateral sums L5..L2 (the upsampled level above is added to the fp32 sum, then stored), P2..P5;
    #   RPN: the shared 3x3 layer's 512-channel output (the logits / deltas are fp32);
    #   box head: the two 1024-wide hidden layers (logits / box deltas are fp32);
    #   mask head: the four 3x3 layers' outputs and the deconvolution's (the 1x1 class filter and the sigmoid are fp32).
    # The fp32-grade modes store fp32 tensors: round_f16=False.
    def _w64(self):
        if getattr(self, "_w64_cache", None) is None:
            self._w64_cache = tuple(_W({k: v.numpy() for k, v in w.t.items()}, torch.float64, folded=True)
                                    for w in (self.w, self.wc, self.wm))
        return self._w64_cache

    @staticmethod
    def _t64(x):
        return x.to(torch.float64) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))

    def stem64(self, images_u8, round_f16=False):
        """uint8 (B,H,W,3) → C1 (B,64,H/4,W/4): mean subtraction, conv1 7×7/2 + BN + ReLU, 3×3/2 max pool."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[0]
        x = np.ascontiguousarray(images_u8).astype(np.float32) - np.asarray(self.cfg.mean_rgb, np.float32)
        with torch.no_grad():
            x = r(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).contiguous())
            x = r(F.relu(w.conv(F.pad(x, (3, 3, 3, 3)), "conv1", stride=2)))
            x = F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=float("-inf")), 3, 2)
        return x.numpy()

    def stage64(self, st, x, round_f16=False):
        """C{st-1} (C1 for st = 2) → C{st}: the stage's residual blocks."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[0]
        with torch.no_grad():
            x = self._t64(x)
            for b in _stage_blocks(self.cfg.architecture)[st]:
                p, first = f"res{st}{b}", b == "a"
                stride = 2 if (first and st > 2) else 1
                y = r(F.relu(w.conv(x, f"{p}_branch2a", stride=stride)))
                y = r(F.relu(w.conv(y, f"{p}_branch2b", padding=1)))
                sc = r(w.conv(x, f"{p}_branch1", stride=stride)) if first else x
                x = r(F.relu(w.conv(y, f"{p}_branch2c") + sc))
        return x.numpy()

    def fpn64(self, feats, round_f16=False):
        """[C2..C5] → [P2..P5]."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[0]
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        with torch.no_grad():
            c2, c3, c4, c5 = (self._t64(c) for c in feats)
            l5 = r(w.conv(c5, "fpn_c5p5"))
            l4 = r(w.conv(c4, "fpn_c4p4") + up(l5))
            l3 = r(w.conv(c3, "fpn_c3p3") + up(l4))
            l2 = r(w.conv(c2, "fpn_c2p2") + up(l3))
            return [r(w.conv(l, f"fpn_p{i + 2}", padding=1)).numpy() for i, l in enumerate((l2, l3, l4, l5))]

    def rpn64(self, pyramid, round_f16=False):
        """[P2..P5] → probabilities (B,A,2), deltas (B,A,4); P6 = P5[::2, ::2]."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[0]
        probs, deltas = [], []
        with torch.no_grad():
            pyr = [self._t64(p) for p in pyramid]
            for p in pyr + [pyr[3][:, :, ::2, ::2]]:
                s = r(F.relu(w.conv(p, "rpn_conv_shared", padding=1)))
                lg = w.conv(s, "rpn_class_raw").permute(0, 2, 3, 1)
                probs.append(F.softmax(lg.reshape(lg.shape[0], -1, 2), dim=-1))
                bb = w.conv(s, "rpn_bbox_pred").permute(0, 2, 3, 1)
                deltas.append(bb.reshape(bb.shape[0], -1, 4))
        return torch.cat(probs, 1).numpy(), torch.cat(deltas, 1).numpy()

    def classifier64(self, pooled, round_f16=False):
        """pooled (n,256,7,7) → probabilities (n,nc), box deltas (n,nc*4)."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[1]
        with torch.no_grad():
            x = self._t64(pooled)
            x = r(F.relu(w.conv(x, "mrcnn_class_conv1")))
            x = r(F.relu(w.conv(x, "mrcnn_class_conv2"))).reshape(x.shape[0], -1)
            logits = F.linear(x, w.t["mrcnn_class_logits/kernel"], w.t["mrcnn_class_logits/bias"])
            bbox = F.linear(x, w.t["mrcnn_bbox_fc/kernel"], w.t["mrcnn_bbox_fc/bias"])
            return F.softmax(logits, dim=-1).numpy(), bbox.numpy()

    def mask64(self, pooled_mask, round_f16=False):
        """pooled_mask (n,256,14,14) → masks (n,nc,28,28)."""
        r = round_to_f16 if round_f16 else _same
        w = self._w64()[2]
        with torch.no_grad():
            x = self._t64(pooled_mask)
            for i in range(1, 5):
                x = r(F.relu(w.conv(x, f"mrcnn_mask_conv{i}", padding=1)))
            x = r(F.relu(F.conv_transpose2d(x, w.t["mrcnn_mask_deconv/kernel"], w.t["mrcnn_mask_deconv/bias"], stride=2)))
            return torch.sigmoid(w.conv(x, "mrcnn_mask")).numpy()

    def trunk_fp64(self, images_u8, round_f16=False):
        """The trunk in float64 (the stages above chained): the ground truth that the engines' summation-order /
        split-precision errors are measured against.  Returns ([P2..P5], probs, deltas) like trunk()."""
        c = [self.stem64(images_u8, round_f16)]
        for st in (2, 3, 4, 5):
            c.append(self.stage64(st, c[-1], round_f16))
        pyr = self.fpn64(c[1:], round_f16)
        probs, deltas = self.rpn64(pyr, round_f16)
        return pyr, probs, deltas

    # ---- Classifier.mlmodel / Mask.mlmodel -----------------------------------------------------
    def classifier_model(self, fmap):
        """feature_map (n,256,7,7) → probabilities (n,nc), bounding_boxes (n, nc*4)."""
        w = self.wc
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(fmap, dtype=np.float32))
            x = F.relu(w.bn(w.conv(x, "mrcnn_class_conv1"), "mrcnn_class_bn1"))
            x = F.relu(w.bn(w.conv(x, "mrcnn_class_conv2"), "mrcnn_class_bn2"))
            x = x.reshape(x.shape[0], -1)
            logits = F.linear(x, w.t["mrcnn_class_logits/kernel"], w.t["mrcnn_class_logits/bias"])
            probs = F.softmax(logits, dim=-1)
            bbox = F.linear(x, w.t["mrcnn_bbox_fc/kernel"], w.t["mrcnn_bbox_fc/bias"])
        return probs.numpy(), bbox.numpy()

    def mask_model(self, fmap):
        """feature_map (n,256,14,14) → masks (n,nc,28,28)."""
        w = self.wm
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(fmap, dtype=np.float32))
            if x.shape[0] == 0:
                return np.zeros((0, self.cfg.num_classes, 2 * x.shape[2], 2 * x.shape[3]), np.float32)
            for i in range(1, 5):
                x = F.relu(w.bn(w.conv(x, f"mrcnn_mask_conv{i}", padding=1), f"mrcnn_mask_bn{i}"))
            x = F.relu(F.conv_transpose2d(x, w.t["mrcnn_mask_deconv/kernel"], w.t["mrcnn_mask_deconv/bias"], stride=2))
            x = torch.sigmoid(w.conv(x, "mrcnn_mask"))
        return x.numpy()

    # ---- stages after the trunk (each usable on its own with taps from the HIP engine) ---------
    def proposals(self, probs, deltas, debug=False):
        c = self.cfg
        return orc.proposal_layer(probs, deltas, self.anchors, c.pre_nms_max_proposals, c.max_proposals,
                                  c.rpn_nms_threshold, c.bounding_box_std_dev, debug=debug)

    def roi_align(self, rois, pyramid, pool):
        c = self.cfg
        pp = c.pyramid_params(pool)
        return orc.pyramid_roi_align(rois, pyramid, pool, pp["imageWidth"], pp["imageHeight"])

    def classify(self, pooled):
        probs, bbox = self.classifier_model(pooled)
        return orc.classifier_postprocess(probs, bbox), probs, bbox

    def detect(self, rois, cls6):
        c = self.cfg
        return orc.detection_layer(rois, cls6, c.max_detections, c.detection_min_confidence,
                                   c.detection_nms_threshold, c.bounding_box_std_dev)

    def masks(self, pooled_mask, detections, out=None, valid_from=None):
        """valid_from: the rows the removeZeros predicate is evaluated on when they differ from what the mask model is
        fed (fp16 engine: the predicate sees the fp32 samples, the model their fp16 rounding)."""
        mapping = orc.mask_valid_rows(pooled_mask if valid_from is None else valid_from)
        m = self.mask_model(pooled_mask[mapping])
        if out is None:
            out = np.zeros((detections.shape[0], m.shape[2] * m.shape[3] if m.size else 784), np.float32)
        return orc.mask_layer_write(m, mapping, detections, out)

    def predict(self, images_u8, taps=False):
        """images (B,H,W,3) uint8 → detections (B,max_det,6), masks (B,max_det,28,28)."""
        pyr, probs, deltas = self.trunk(images_u8)
        B = probs.shape[0]
        dets, masks, tap = [], [], []
        for b in range(B):
            pb = [p[b] for p in pyr]
            rois = self.proposals(probs[b], deltas[b])
            pooled = self.roi_align(rois, pb, self.cfg.classifier_pool_size)
            cls6, cprobs, cbbox = self.classify(pooled)
            det = self.detect(rois, cls6)
            pooled_m = self.roi_align(det, pb, self.cfg.mask_pool_size)
            mk = self.masks(pooled_m, det)
            dets.append(det)
            masks.append(mk.reshape(det.shape[0], 2 * self.cfg.mask_pool_size, 2 * self.cfg.mask_pool_size))
            if taps:
                tap.append({"rois": rois, "pooled": pooled, "cls6": cls6, "probs": cprobs, "bbox": cbbox,
                            "pooled_mask": pooled_m})
        out = (np.stack(dets), np.stack(masks))
        if taps:
            return out + ({"pyramid": pyr, "rpn_probs": probs, "rpn_deltas": deltas, "per_image": tap},)
        return out


def load_oracle_model(model_dir: str, cfg=None) -> OracleMaskRCNN:
    anchors_mod = importlib.import_module("mask-rcnn-coreml_amd.anchors")
    config_mod = importlib.import_module("mask-rcnn-coreml_amd.config")
    meta, main = weights_mod.read_mrcw(os.path.join(model_dir, "MaskRCNN.mrcw"))
    _, cls = weights_mod.read_mrcw(os.path.join(model_dir, "Classifier.mrcw"))
    _, msk = weights_mod.read_mrcw(os.path.join(model_dir, "Mask.mrcw"))
    if cfg is None:
        cfg = config_mod.ModelConfig(architecture=meta["architecture"],
                                     input_image_shape=(meta["image_height"], meta["image_width"], 3),
                                     num_classes=meta["num_classes"],
                                     pre_nms_max_proposals=meta["pre_nms_max_proposals"],
                                     max_proposals=meta["max_proposals"],
                                     max_detections=meta["DetectionLayer.maxDetections"])
    anchors = anchors_mod.read_anchors_bin(os.path.join(model_dir, "anchors.bin"), cfg.num_anchors())
    return OracleMaskRCNN(cfg, main, cls, msk, anchors)
