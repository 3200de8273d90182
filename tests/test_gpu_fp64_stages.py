"""Every compute mode pinned stage by stage against a float64 evaluation of the same graph (oracle/network.py: stem64 ... mask64).

Each stage of the float64 reference is fed THE GPU'S OWN TAP of its input (u8 -> C1, C1 -> C2, ..., C2..C5 -> P2..P5, P -> RPN,
pooled -> box head, pooled_mask -> mask head), so a failure names the stage and a bound only has to absorb one stage of rounding.
The fp32-grade modes (f32, f32s, f32x3 with and without stored split exponents) are also compared with one float64 trunk per image;
the fp16 mode is compared with the float64 reference that rounds every tensor the mode stores to fp16 (round_f16=True).

Error metric, per output channel: max |x - ref|_c / max(max |ref|_c, FLOOR * max |ref|) — a border or tile fault in a small-magnitude
channel does not hide behind the tensor's maximum.  FLOOR = 1e-2: a channel whose whole range lies below 1 % of the tensor's is
measured at 1 % of the tensor's scale (below that, the cancellation of its pre-activation dominates its own maximum, not the
kernel's arithmetic).  Probabilities and mask values: absolute.

The pinned predicts run with the conv profile on: every tile class a batch-8 full-size predict launches in a mode must have run in a
pinned predict of that mode, so that a policy change that moves a layer onto an unpinned form fails here.
"""
import importlib
import json
import os
import shutil

import numpy as np
import pytest

from conftest import rand_images

pytestmark = pytest.mark.gpu

FLOOR = 1e-2
FP32_MODES = ("f32", "f32s", "f32x3cal", "f32x3")
MODES = FP32_MODES + ("f16",)
STAGES = ("C1", "C2", "C3", "C4", "C5", "P2", "P3", "P4", "P5", "rpn_probs", "rpn_deltas", "cls_probs", "cls_bbox", "mask")
TRUNK = tuple("T:" + s for s in STAGES[:11])

# BOUNDS[mode][stage] = (bound, worst value measured on an MI355X over every pinned image of every config).  "T:<stage>": the whole
# trunk against one float64 evaluation per image.  f32x3cal: loaded with no compute dtype from an artefact with stored split
# exponents (MRCNN_DEFAULT, the headline path).  A bound is 4x the measured value, capped at the ceiling of its class (fp32-grade:
# 2e-5 per stage and for probabilities / mask values, 1e-5 whole trunk, 3e-5 whole-trunk rpn_probs; f16: 5e-3 per stage) where the
# measurement leaves 25 % below it.  ABOVE_CEILING lists where it does not; those bounds are 2x the measured value.  They are the
# deep stages, measured per channel: C4 (6 / 23 residual blocks) and C5 chain dozens of layers inside one stage and the per-channel
# metric scores each channel against its own range; the torch-CPU fp32 network itself measures 8e-6 (C4) and 7e-6 (C5) on this
# metric at R50 128^2 (tests/test_oracle_fp64_stages.py pins it below 4e-6 at P level), and in the f16 mode the rounded reference
# and the kernels part ways by one fp16 rounding flip per layer.  The box head's probabilities in f32 follow its K = 12 544 inner
# product in plain fp32 (the split modes are 3x closer).  f16 whole trunk: no ceiling (4x measured).
BOUNDS = {
    "f32": {
        "C1": (2.9e-06, 7.24e-07), "C2": (1.5e-05, 3.61e-06), "C3": (2.0e-05, 8.52e-06), "C4": (5.0e-05, 2.47e-05),
        "C5": (4.5e-05, 2.21e-05), "P2": (2.0e-05, 5.46e-06), "P3": (2.0e-05, 7.40e-06), "P4": (2.0e-05, 5.96e-06),
        "P5": (2.0e-05, 5.66e-06), "rpn_probs": (2.0e-05, 7.37e-06), "rpn_deltas": (1.1e-05, 2.61e-06), "cls_probs": (1.2e-04, 5.69e-05),
        "cls_bbox": (2.0e-05, 1.13e-05), "mask": (2.0e-05, 7.06e-06), "T:C1": (2.9e-06, 7.24e-07), "T:C2": (1.0e-05, 3.67e-06),
        "T:C3": (3.4e-05, 1.69e-05), "T:C4": (5.3e-05, 2.60e-05), "T:C5": (7.6e-05, 3.76e-05), "T:P2": (1.7e-05, 8.10e-06),
        "T:P3": (1.7e-05, 8.50e-06), "T:P4": (1.0e-05, 7.97e-06), "T:P5": (2.0e-05, 9.69e-06), "T:rpn_probs": (3.0e-05, 1.15e-05),
        "T:rpn_deltas": (1.0e-05, 4.25e-06),
    },
    "f32s": {
        "C1": (1.9e-06, 4.71e-07), "C2": (1.8e-05, 4.50e-06), "C3": (2.0e-05, 5.21e-06), "C4": (2.0e-05, 1.29e-05),
        "C5": (5.8e-05, 2.87e-05), "P2": (1.5e-05, 3.51e-06), "P3": (1.7e-05, 4.03e-06), "P4": (1.3e-05, 3.08e-06),
        "P5": (1.3e-05, 3.02e-06), "rpn_probs": (1.5e-05, 3.52e-06), "rpn_deltas": (5.2e-06, 1.29e-06), "cls_probs": (3.4e-05, 1.69e-05),
        "cls_bbox": (1.2e-05, 2.83e-06), "mask": (1.6e-05, 3.87e-06), "T:C1": (1.9e-06, 4.71e-07), "T:C2": (1.0e-05, 4.34e-06),
        "T:C3": (1.0e-05, 5.94e-06), "T:C4": (3.1e-05, 1.52e-05), "T:C5": (6.3e-05, 3.12e-05), "T:P2": (1.0e-05, 5.16e-06),
        "T:P3": (1.0e-05, 5.33e-06), "T:P4": (1.0e-05, 5.01e-06), "T:P5": (1.0e-05, 5.69e-06), "T:rpn_probs": (2.5e-05, 6.16e-06),
        "T:rpn_deltas": (9.8e-06, 2.44e-06),
    },
    "f32x3cal": {
        "C1": (1.9e-06, 4.71e-07), "C2": (1.3e-05, 3.25e-06), "C3": (2.0e-05, 6.26e-06), "C4": (2.0e-05, 1.49e-05),
        "C5": (2.0e-05, 1.25e-05), "P2": (1.5e-05, 3.57e-06), "P3": (1.5e-05, 3.60e-06), "P4": (1.2e-05, 2.86e-06),
        "P5": (1.4e-05, 3.48e-06), "rpn_probs": (1.3e-05, 3.11e-06), "rpn_deltas": (5.0e-06, 1.23e-06), "cls_probs": (3.6e-05, 1.79e-05),
        "cls_bbox": (1.3e-05, 3.17e-06), "mask": (2.0e-05, 5.07e-06), "T:C1": (1.9e-06, 4.71e-07), "T:C2": (1.0e-05, 4.34e-06),
        "T:C3": (1.0e-05, 6.01e-06), "T:C4": (3.6e-05, 1.77e-05), "T:C5": (6.0e-05, 2.96e-05), "T:P2": (1.0e-05, 5.57e-06),
        "T:P3": (1.0e-05, 5.11e-06), "T:P4": (1.0e-05, 5.37e-06), "T:P5": (1.0e-05, 6.24e-06), "T:rpn_probs": (2.7e-05, 6.67e-06),
        "T:rpn_deltas": (9.7e-06, 2.41e-06),
    },
    "f32x3": {
        "C1": (1.9e-06, 4.71e-07), "C2": (2.0e-05, 8.19e-06), "C3": (2.0e-05, 5.65e-06), "C4": (2.0e-05, 1.50e-05),
        "C5": (2.0e-05, 1.39e-05), "P2": (1.4e-05, 3.45e-06), "P3": (1.4e-05, 3.42e-06), "P4": (1.3e-05, 3.06e-06),
        "P5": (1.4e-05, 3.31e-06), "rpn_probs": (1.5e-05, 3.73e-06), "rpn_deltas": (4.8e-06, 1.18e-06), "cls_probs": (2.0e-05, 1.45e-05),
        "cls_bbox": (1.4e-05, 3.29e-06), "mask": (1.6e-05, 3.99e-06), "T:C1": (1.9e-06, 4.71e-07), "T:C2": (1.0e-05, 5.10e-06),
        "T:C3": (1.0e-05, 6.75e-06), "T:C4": (3.4e-05, 1.66e-05), "T:C5": (5.6e-05, 2.76e-05), "T:P2": (1.0e-05, 5.18e-06),
        "T:P3": (1.0e-05, 5.46e-06), "T:P4": (1.0e-05, 5.72e-06), "T:P5": (1.0e-05, 5.68e-06), "T:rpn_probs": (2.8e-05, 6.91e-06),
        "T:rpn_deltas": (9.6e-06, 2.39e-06),
    },
    "f16": {
        "C1": (2.8e-03, 6.93e-04), "C2": (5.0e-03, 2.37e-03), "C3": (1.4e-02, 6.62e-03), "C4": (5.5e-02, 2.72e-02),
        "C5": (1.7e-02, 8.41e-03), "P2": (3.9e-03, 9.67e-04), "P3": (3.9e-03, 9.62e-04), "P4": (3.7e-03, 9.12e-04),
        "P5": (3.9e-03, 9.62e-04), "rpn_probs": (2.5e-03, 6.05e-04), "rpn_deltas": (8.5e-04, 2.10e-04), "cls_probs": (5.0e-03, 3.56e-03),
        "cls_bbox": (3.3e-03, 8.08e-04), "mask": (5.0e-03, 1.85e-03), "T:C1": (2.8e-03, 6.93e-04), "T:C2": (1.4e-02, 3.40e-03),
        "T:C3": (4.5e-02, 1.11e-02), "T:C4": (1.3e-01, 3.06e-02), "T:C5": (2.4e-01, 5.92e-02), "T:P2": (3.8e-02, 9.33e-03),
        "T:P3": (3.4e-02, 8.42e-03), "T:P4": (3.3e-02, 8.23e-03), "T:P5": (4.2e-02, 1.05e-02), "T:rpn_probs": (3.5e-02, 8.59e-03),
        "T:rpn_deltas": (1.4e-02, 3.34e-03),
    },
}
ABOVE_CEILING = {
    "f32": ("C4", "C5", "cls_probs", "T:C3", "T:C4", "T:C5", "T:P2", "T:P3", "T:P5"),
    "f32s": ("C5", "cls_probs", "T:C4", "T:C5"),
    "f32x3cal": ("cls_probs", "T:C4", "T:C5"),
    "f32x3": ("T:C4", "T:C5"),
    "f16": ("C3", "C4", "C5"),
}


def _ceiling(mode, stage):
    if mode == "f16":
        return None if stage.startswith("T:") else 5e-3
    return 3e-5 if stage == "T:rpn_probs" else 1e-5 if stage.startswith("T:") else 2e-5


# (architecture, size, batch, pinned images, modes)
CONFIGS = {
    "r50_128": ("resnet50", 128, 3, (2,), MODES),
    "r101_1024": ("resnet101", 1024, 2, (0, 1), MODES),
    "r50_1024": ("resnet50", 1024, 2, (1,), ("f32x3cal", "f16")),
}

models = importlib.import_module("mask-rcnn-coreml_amd.models")


def _images(B, S, seed):
    """Image 0 random; images 1.. random with flat 0 and 255 blocks (one on a tile boundary, one off it)."""
    x = rand_images(B, S, S, seed=seed)
    for b in range(1, B):
        x[b, : S // 4, : S // 4] = 0
        x[b, S // 2 + 3: S // 2 + S // 5, S // 8 + 5: S - S // 8] = 255
    return x


def chan_err(x, ref, axis=1):
    from oracle.network import channel_error
    return channel_error(x, ref, axis, FLOOR)


def abs_err(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max())


class _Ctx:
    def __init__(self, tmp_path_factory):
        self.tmp = tmp_path_factory
        self.dirs, self.oms, self.trunks, self.runs = {}, {}, {}, {}
        self.cover = {m: set() for m in MODES}

    def model_dir(self, key, calibrated=False):
        if key not in self.dirs:
            pkg = importlib.import_module("mask-rcnn-coreml_amd")
            weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
            arch, S, B, _, _ = CONFIGS[key]
            cfg = pkg.ModelConfig(architecture=arch, input_image_shape=(S, S, 3), **({} if S > 128 else dict(
                num_classes=21, pre_nms_max_proposals=300, max_proposals=64, max_detections=16)))
            d = str(self.tmp.mktemp("fp64_" + key))
            weights.save_synthetic_models(d, cfg, seed=0)
            self.dirs[key] = (d, cfg)
        if calibrated and key + "/cal" not in self.dirs:
            convert = importlib.import_module("mask-rcnn-coreml_amd.convert")
            d, cfg = self.dirs[key]
            dc = str(self.tmp.mktemp("fp64_" + key + "_cal"))
            shutil.copytree(d, dc, dirs_exist_ok=True)
            convert.calibrate_artefact(dc, self.images(key), verbose=False)       # what `convert --calibrate` does
            self.dirs[key + "/cal"] = (dc, cfg)
        return self.dirs[key + "/cal" if calibrated else key]

    def images(self, key):
        _, S, B, _, _ = CONFIGS[key]
        return _images(B, S, seed=11 + S)

    def oracle(self, key):
        if key not in self.oms:
            from oracle.network import load_oracle_model
            self.oms[key] = load_oracle_model(self.model_dir(key)[0])
        return self.oms[key]

    def trunk(self, key, b, f16):
        """The whole float64 trunk of image b: C1..C5, P2..P5, probs, deltas (shared by every mode of its precision class)."""
        k = (key, b, f16)
        if k not in self.trunks:
            om = self.oracle(key)
            c = [om.stem64(self.images(key)[b:b + 1], f16)]
            for st in (2, 3, 4, 5):
                c.append(om.stage64(st, c[-1], f16))
            p = om.fpn64(c[1:], f16)
            probs, deltas = om.rpn64(p, f16)
            self.trunks[k] = dict(zip(STAGES[:9], c + p), rpn_probs=probs[0], rpn_deltas=deltas[0])
        return self.trunks[k]

    def load(self, key, mode, max_batch):
        if mode == "f32x3cal":
            d, cfg = self.model_dir(key, calibrated=True)
            m = models.load_maskrcnn(d, max_batch=max_batch)                   # no compute dtype: MRCNN_DEFAULT
            assert m.get_int("compute_dtype") == 6 and m.get_int("split_calibrated") == 1
            return m, cfg
        d, cfg = self.model_dir(key)
        return models.load_maskrcnn(d, max_batch=max_batch, compute_dtype=mode), cfg

    def profiled_predict(self, m, mode, images):
        m.conv_profile_enable(True)
        m.predict(images)
        m.conv_profile_enable(False)
        used = {t for t, v in m.conv_profile().items() if v[0] > 0}
        self.cover[mode] |= used
        return used


TAP_NAMES = ("C1", "C2", "C3", "C4", "C5", "P2", "P3", "P4", "P5", "rpn_probs", "rpn_deltas", "pooled", "cls_probs", "cls_bbox",
             "detections", "pooled_mask", "mask_row_flags", "mask")


def _taps(m, b):
    return {n: m.read_tensor(n, b) for n in TAP_NAMES}


def _stage_errors(ctx, key, mode, images, b, t, cfg):
    """{stage: error} of image b's taps t: every stage fed the GPU's own tap of its input."""
    om = ctx.oracle(key)
    f16 = mode == "f16"
    H = cfg.image_height
    A = cfg.num_anchors()
    chw = lambda x, h, c: x.reshape(h, -1, c).transpose(2, 0, 1)[None]
    C = {"C1": chw(t["C1"], H // 4, 64)}
    for st in (2, 3, 4, 5):
        C[f"C{st}"] = chw(t[f"C{st}"], H >> st, 256 << (st - 2))
    shapes = cfg.feature_shapes()
    P = [chw(t[f"P{l + 2}"], shapes[l][0], 256) for l in range(4)]
    probs, deltas = t["rpn_probs"].reshape(A, 2), t["rpn_deltas"].reshape(A, 4)
    e = {"C1": chan_err(C["C1"], om.stem64(images[b:b + 1], f16))}
    for st in (2, 3, 4, 5):
        e[f"C{st}"] = chan_err(C[f"C{st}"], om.stage64(st, C[f"C{st - 1}"], f16))
    for l, ref in enumerate(om.fpn64([C[f"C{st}"] for st in (2, 3, 4, 5)], f16)):
        e[f"P{l + 2}"] = chan_err(P[l], ref)
    rp, rd = om.rpn64(P, f16)
    e["rpn_probs"], e["rpn_deltas"] = abs_err(probs, rp[0]), chan_err(deltas, rd[0])
    ps, pm, nc = cfg.classifier_pool_size, cfg.mask_pool_size, cfg.num_classes
    pooled = t["pooled"].reshape(-1, ps, ps, 256).transpose(0, 3, 1, 2)
    cp, cb = om.classifier64(pooled, f16)
    e["cls_probs"] = abs_err(t["cls_probs"].reshape(-1, nc), cp)
    e["cls_bbox"] = chan_err(t["cls_bbox"].reshape(-1, 4 * nc), cb)
    # mask head on the rows the engine's removeZeros predicate kept, each detection's class selected as the engine does
    from oracle import oracle as orc
    det = t["detections"].reshape(cfg.max_detections, 6)
    rows = np.flatnonzero(t["mask_row_flags"] > 0)
    assert rows.size > 0, "no mask rows: the mask head was not exercised"
    pmk = t["pooled_mask"].reshape(-1, pm, pm, 256).transpose(0, 3, 1, 2)[rows]
    want = orc.mask_layer_write(om.mask64(pmk, f16), rows, det, np.zeros((cfg.max_detections, 4 * pm * pm), np.float32))
    e["mask"] = abs_err(t["mask"].reshape(cfg.max_detections, -1), want)
    # the whole trunk against one float64 evaluation of the image
    ref = ctx.trunk(key, b, f16)
    for s in STAGES[:9]:
        e["T:" + s] = chan_err(C[s] if s[0] == "C" else P[int(s[1]) - 2], ref[s])
    e["T:rpn_probs"], e["T:rpn_deltas"] = abs_err(probs, ref["rpn_probs"]), chan_err(deltas, ref["rpn_deltas"])
    return e


def pinned_run(ctx, key, mode):
    """Predict the config's batch in `mode` (conv profile on), pin its pinned images stage by stage; cached per (config, mode)."""
    if (key, mode) in ctx.runs:
        return ctx.runs[(key, mode)]
    _, S, B, pin, _ = CONFIGS[key]
    images = ctx.images(key)
    m, cfg = ctx.load(key, mode, B)
    ctx.profiled_predict(m, mode, images)
    taps = {b: _taps(m, b) for b in pin}
    if S > 128:
        # the single-image path (the reference's only operating point: other grid sizes, other forms) on the last image:
        # bit-identical to that image in the batch, so the float64 pin below covers it
        ctx.profiled_predict(m, mode, images[B - 1:B])
        one = _taps(m, 0)
        for n in TAP_NAMES:
            assert np.array_equal(one[n].view(np.uint32), taps[B - 1][n].view(np.uint32)), f"{key} {mode}: batch 1 differs from batch {B} at {n}"
    del m
    errs = {}
    for b in pin:
        for s, v in _stage_errors(ctx, key, mode, images, b, taps[b], cfg).items():
            errs[s] = max(errs.get(s, 0.0), v)
    print(f"\nFP64_STAGES {json.dumps({'config': key, 'mode': mode, 'errors': errs})}")
    ctx.runs[(key, mode)] = errs
    return errs


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    return _Ctx(tmp_path_factory)


def _over(errs, mode):
    return {s: (v, BOUNDS[mode][s][0]) for s, v in errs.items() if not v <= BOUNDS[mode][s][0]}


def test_bounds_table_keeps_its_ceilings():
    for mode, table in BOUNDS.items():
        assert set(table) == set(STAGES + TRUNK), mode
        for stage, (bound, measured) in table.items():
            c = _ceiling(mode, stage)
            assert measured < bound, (mode, stage)
            assert c is None or bound <= c or stage in ABOVE_CEILING[mode], (mode, stage, bound, c)


@pytest.mark.parametrize("key,mode", [(k, m) for k, c in CONFIGS.items() for m in c[4]])
def test_stages_against_float64(ctx, key, mode):
    errs = pinned_run(ctx, key, mode)
    assert set(errs) == set(STAGES + TRUNK)
    over = _over(errs, mode)
    assert not over, f"{key} {mode}: stages above their float64 bound (error, bound): {over}"


def test_every_tile_class_of_a_batch8_headline_predict_is_pinned(ctx):
    """The tile classes a batch-8 full-size (R101 1024^2) predict launches in each mode all ran in a pinned predict of that mode."""
    for key, c in CONFIGS.items():
        for mode in c[4]:
            pinned_run(ctx, key, mode)
    images = _images(8, 1024, seed=3)
    for mode in MODES:
        m, _ = ctx.load("r101_1024", mode, 8)
        m.predict(images)
        m.conv_profile_enable(True)
        m.predict(images)
        m.conv_profile_enable(False)
        used = {t for t, v in m.conv_profile().items() if v[0] > 0}
        del m
        print(f"\nFP64_COVER {mode}: batch 8 {sorted(used)}, pinned {sorted(ctx.cover[mode])}")
        assert used, mode
        assert used <= ctx.cover[mode], f"{mode}: tile classes {sorted(used - ctx.cover[mode])} of a batch-8 predict are not pinned"


def test_a_bn_fold_off_by_1e5_is_flagged(ctx, tmp_path):
    """Negative control: the small model saved with bn_eps = 1.02e-3 in MaskRCNN.mrcw while the float64 reference folds 1e-3.
    With variances ~1 (synthetic BN: 0.8 .. 1.2) every BN scale of the trunk shrinks by 0.5 * 2e-5 / (1 + 1e-3) ~ 1e-5 relative — a
    fold off by 1e-5 per layer.  The comparator flags it; the suite's fp32 trunk bar (TRUNK_RTOL = 5e-4 against the torch-CPU fp32
    network, tests/test_gpu_engine.py) does not."""
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    d, cfg = ctx.model_dir("r50_128")
    bad = str(tmp_path / "eps")
    shutil.copytree(d, bad)
    meta, tensors = weights.read_mrcw(os.path.join(bad, "MaskRCNN.mrcw"))
    assert meta["bn_eps"] == pytest.approx(1e-3)
    meta["bn_eps"] = 1.02e-3
    weights.write_mrcw(os.path.join(bad, "MaskRCNN.mrcw"), meta, tensors)
    images = ctx.images("r50_128")
    b = CONFIGS["r50_128"][3][0]
    m = models.load_maskrcnn(bad, max_batch=images.shape[0], compute_dtype="f32x3")
    m.predict(images)
    t = _taps(m, b)
    errs = _stage_errors(ctx, "r50_128", "f32x3", images, b, t, cfg)
    print(f"\nFP64_CONTROL {json.dumps(errs)}")
    over = _over(errs, "f32x3")
    assert over, "a BN fold off by 1e-5 per layer passed every float64 bound"
    # ... while the existing fp32 bar passes it
    om = ctx.oracle("r50_128")
    pyr, oprobs, odeltas = om.trunk(images[b:b + 1])
    rel = lambda a, r: float(np.abs(a - r).max() / np.abs(r).max())
    for l, (h, w) in enumerate(cfg.feature_shapes()[:4]):
        assert rel(t[f"P{l + 2}"].reshape(h, w, 256).transpose(2, 0, 1), pyr[l][0]) < 5e-4
    assert rel(t["rpn_deltas"].reshape(-1, 4), odeltas[0]) < 5e-4
    assert np.abs(t["rpn_probs"].reshape(-1, 2) - oprobs[0]).max() < 5e-4
