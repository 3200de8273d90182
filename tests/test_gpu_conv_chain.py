"""The chained pair of the split modes (kernels_conv_chain.hip) against the two launches it replaces.

P = a bottleneck's branch2c (1x1, C -> 4C, + residual or the stage's shortcut convolution, ReLU), Q = the NEXT block's branch2a
(1x1, 4C -> C, ReLU).  The chained launch stores y = P's output and computes t1 = Q's output from the tile while it is on chip.
Which form runs is a launch-time policy (the grid size), so both outputs must agree with conv_forward x 2 BIT FOR BIT; the two
launches themselves are held against a float64 evaluation, which is what makes the bit-identity mean something.
"""
import ctypes
import functools
import importlib
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")

DT = {"f32s": L.F32S, "f32x3": L.F32X3}
FP16_LIMIT = 65504.0


def chain(case, dtype, chained, in_place):
    B, H, W, C = case["t2"].shape
    keep = {k: (None if v is None else np.ascontiguousarray(v, np.float32)) for k, v in case.items() if k not in ("cs", "ss")}
    p = lambda k: None if keep[k] is None else keep[k].ctypes.data
    y = np.empty((B, H, W, 4 * C), np.float32)
    t1 = np.empty((B, H, W, C), np.float32)
    L.check(L.lib().mrcnn_conv_chain_nhwc(p("t2"), B, H, W, C, p("w3"), p("s3"), p("h3"), p("x"), p("xs"), case["cs"], case["ss"], p("ws"), p("s_s"), p("h_s"),
                                           p("w1"), p("s1"), p("h1"), DT[dtype], int(chained), int(in_place), y.ctypes.data, t1.ctypes.data))
    f = ctypes.c_int(-1)
    L.check(L.lib().mrcnn_test_last_range_flag(ctypes.byref(f)))
    return y, t1, f.value


def _acts(rng, shape):
    """post-ReLU activations with a spread of magnitudes: a third zero, the rest |n| * 2^u, u in [-7, 2] (many below 0.5: the third part matters)"""
    a = np.abs(rng.standard_normal(shape)) * np.exp2(rng.uniform(-7, 2, shape))
    return np.where(rng.random(shape) < 0.33, 0.0, a).astype(np.float32)


def _bn(rng, n):
    """scale with both signs, shift around zero: ReLU zeroes a good share of the outputs"""
    s = (1.0 + 0.1 * rng.standard_normal(n)) * np.where(rng.random(n) < 0.4, -1.0, 1.0)
    return s.astype(np.float32), (0.3 * rng.standard_normal(n)).astype(np.float32)


def make(C, B, H, W, entry, seed):
    rng = np.random.default_rng(seed)
    c = {"t2": _acts(rng, (B, H, W, C)), "cs": 0, "ss": 1, "x": None, "xs": None, "ws": None, "s_s": None, "h_s": None}
    c["w3"] = (rng.standard_normal((4 * C, C)) * np.sqrt(2.0 / C)).astype(np.float32)
    c["s3"], c["h3"] = _bn(rng, 4 * C)
    c["w1"] = (rng.standard_normal((C, 4 * C)) * np.sqrt(2.0 / (4 * C))).astype(np.float32)
    c["s1"], c["h1"] = _bn(rng, C)
    if entry:          # C = 64: stride-1 shortcut from 64 channels (C2); C = 128: stride-2 shortcut from 256 channels (C3)
        c["cs"], c["ss"] = (64, 1) if C == 64 else (256, 2)
        c["xs"] = _acts(rng, (B, H * c["ss"], W * c["ss"], c["cs"]))
        c["ws"] = (rng.standard_normal((4 * C, c["cs"])) * np.sqrt(2.0 / c["cs"])).astype(np.float32)
        c["s_s"], c["h_s"] = _bn(rng, 4 * C)
    else:
        c["x"] = _acts(rng, (B, H, W, 4 * C))
    return c


def ref64(case, y_gpu):
    """float64 evaluation of both layers on the fp16-rounded filters; Q is fed the GPU's own y (stage by stage)"""
    h = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float64)
    f = lambda a: np.asarray(a, np.float64)
    B, H, W, C = case["t2"].shape
    acc = f(case["t2"]).reshape(-1, C) @ h(case["w3"]).T * f(case["s3"]) + f(case["h3"])
    if case["x"] is not None:
        res = f(case["x"]).reshape(-1, 4 * C)
    else:
        ss = case["ss"]
        res = f(case["xs"])[:, ::ss, ::ss, :].reshape(-1, case["cs"]) @ h(case["ws"]).T * f(case["s_s"]) + f(case["h_s"])
    y = np.maximum(acc + res, 0.0).reshape(B, H, W, 4 * C)
    t1 = np.maximum(f(y_gpu).reshape(-1, 4 * C) @ h(case["w1"]).T * f(case["s1"]) + f(case["h1"]), 0.0).reshape(B, H, W, C)
    return y, t1


# C, B, H, W, entry form — M = 288: two full 128-row tiles and a ragged one, a tile across the image boundary; M = 64: less than a tile;
# the entry forms of C2 (stride-1 shortcut, 64 channels) and C3 (stride-2 shortcut from 256 channels at 24 x 24)
CASES = [(64, 2, 12, 12, False), (128, 2, 12, 12, False), (64, 1, 8, 8, False), (128, 1, 8, 8, False), (64, 2, 12, 12, True), (128, 2, 12, 12, True)]
# the C = 64 form is persistent: one block of eight waves per CU, a wave walks 32-row tiles 256 rows x the grid apart.  H = W = None: a square sized
# on the device so that some waves take a SECOND tile and the last one is ragged (what a wave carries from one tile into the next: Q's sums, the LDS
# tile, the watch); bit-identity only — the small cases hold the two launches against float64
SECOND_TILE = (64, 1, None, None, False)


def _second_tile_side():
    """H = W with H * W between 256 and 1024 rows beyond one 256-row tile per CU and no multiple of 32 (256 CUs: 257 x 257 = 66049 rows)"""
    import torch
    rows = 256 * torch.cuda.get_device_properties(0).multi_processor_count
    return next(s for s in range(1, 1 << 15) if rows + 256 <= s * s <= rows + 1024 and (s * s) % 32)


@functools.lru_cache(maxsize=None)
def _case(C, B, H, W, entry):
    return make(C, B, H, W, entry, seed=C + 7 * B + H + (100 if entry else 0))


@functools.lru_cache(maxsize=None)
def _two_launches(C, B, H, W, entry, dtype, in_place):
    y, t1, flag = chain(_case(C, B, H, W, entry), dtype, False, in_place)
    y.setflags(write=False); t1.setflags(write=False)
    return y, t1, flag


def _same_bits(a, b, what):
    nz = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    assert nz.size == 0, f"{what}: {nz.size} of {a.size} outputs differ, first at {np.unravel_index(nz[0], a.shape)}: {a.flat[nz[0]]} vs {b.flat[nz[0]]}"


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("C,B,H,W,entry", CASES + [SECOND_TILE])
def test_chained_equals_the_two_launches_bitwise(C, B, H, W, entry, dtype, in_place):
    if H is None:
        H = W = _second_tile_side()
    y0, t0, f0 = _two_launches(C, B, H, W, entry, dtype, in_place)
    y1, t1, f1 = chain(_case(C, B, H, W, entry), dtype, True, in_place)
    assert np.isfinite(y1).all() and np.isfinite(t1).all()
    assert (y0 == 0).mean() > 0.1 and (t0 == 0).mean() > 0.1 and (y0 > 0).mean() > 0.1 and (t0 > 0).mean() > 0.1      # ReLU cuts a good share of both
    _same_bits(y1, y0, "y")
    _same_bits(t1, t0, "t1")
    assert f1 == f0 == 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("C,B,H,W,entry", CASES)
def test_the_two_launches_against_float64(C, B, H, W, entry, dtype):
    y0, t0, _ = _two_launches(C, B, H, W, entry, dtype, 0)
    ry, rt = ref64(_case(C, B, H, W, entry), y0)
    tol = {"f32s": 2e-5, "f32x3": 1e-5}[dtype]          # tests/test_gpu_conv_kernels.py's bound for these modes
    ey, et = np.abs(y0 - ry).max(), np.abs(t0 - rt).max()
    print(f"C {C} B {B} {H}x{W} entry {entry} {dtype}: y err {ey:.3e} of max {np.abs(ry).max():.3e}, t1 err {et:.3e} of max {np.abs(rt).max():.3e}")
    assert ey <= tol * max(1.0, np.abs(ry).max()), (ey, np.abs(ry).max())
    assert et <= tol * max(1.0, np.abs(rt).max()), (et, np.abs(rt).max())


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("C", [64, 128])
def test_watchdog_words_agree(C, dtype):
    base = _case(C, 2, 12, 12, False)
    # a single y element past the fp16 range: one residual element (ragged last tile, second image)
    hot_y = dict(base)
    hot_y["x"] = base["x"].copy()
    hot_y["x"][1, 11, 5, 3 * C + 17] = 70000.0
    hot_y["s3"] = np.abs(base["s3"])
    # ... only in t1: one column's shift
    hot_t = dict(base)
    hot_t["h1"] = base["h1"].copy()
    hot_t["h1"][C - 3] = 70000.0
    # just below the limit in both
    warm = dict(hot_y)
    warm["x"] = base["x"].copy()
    warm["x"][1, 11, 5, 3 * C + 17] = 64000.0
    warm["h1"] = base["h1"].copy()
    warm["h1"][C - 3] = 60000.0
    warm["s1"] = base["s1"].copy()
    warm["s1"][C - 3] = 1e-3
    for case, want, name in ((hot_y, 1, "y"), (hot_t, 1, "t1"), (warm, 0, "below")):
        y0, t0, f0 = chain(case, dtype, False, 1)
        y1, t1, f1 = chain(case, dtype, True, 1)
        if name == "y":
            assert (np.abs(y0) >= FP16_LIMIT).sum() == 1
        if name == "t1":
            assert np.abs(y0).max() < FP16_LIMIT and np.abs(t0).max() >= FP16_LIMIT
        if name == "below":
            assert 60000.0 < np.abs(y0).max() < FP16_LIMIT and 59000.0 < np.abs(t0).max() < FP16_LIMIT
        _same_bits(y1, y0, name + ": y")
        _same_bits(t1, t0, name + ": t1")
        assert f0 == want and f1 == want, (name, f0, f1)


@pytest.mark.parametrize("mode", ["f32x3", "f32s"])
def test_in_the_model_the_chain_changes_launches_and_nothing_else(mode):
    """The small ResNet-50 of test_gpu_bench_contract.py (256^2, batch 2) with "conv_chain" 0 (two launches) and 2 (chained at every grid size):
    detections, masks and the C2 / C3 taps bit for bit, five conv launches fewer (C2: a->b, b->c; C3: a->b, b->c, c->d), the same algorithmic
    flops in the backbone and over all classes — also with stored split exponents."""
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(256, 256, 3), num_classes=21, pre_nms_max_proposals=500, max_proposals=64, max_detections=16)
    d = tempfile.mkdtemp(prefix="mrcnn_chain_")
    weights.save_synthetic_models(d, cfg, seed=0, forced_load=True)
    img = np.random.default_rng(0).integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
    got = {}
    try:
        for calib in (False, True):
            for knob in (0, 2):
                L.check(L.lib().mrcnn_debug_set(b"conv_chain", knob))
                m = models.load_maskrcnn(d, max_batch=2, compute_dtype=mode)
                if calib:
                    m.calibrate_split(img)
                det, masks = m.predict(img)
                m.conv_profile_enable(True)
                m.predict(img)
                m.conv_profile_enable(False)
                tiles, groups = m.conv_profile(), m.conv_profile_groups()
                got[calib, knob] = (det.copy(), np.asarray(masks).copy(), [m.read_tensor(n, b).copy() for n in ("C2", "C3") for b in range(2)],
                                    sum(v[0] for v in tiles.values()), groups["backbone"][2], sum(v[2] for v in tiles.values()))
                del m
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_chain", 1))
    for calib in (False, True):
        two, one = got[calib, 0], got[calib, 2]
        assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)), calib
        assert np.array_equal(one[1], two[1]), calib
        for a, b in zip(one[2], two[2]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), calib
        assert two[3] - one[3] == 5, (calib, two[3], one[3])
        assert one[4] == two[4] and one[5] == two[5], (calib, one[4:], two[4:])
