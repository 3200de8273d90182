"""The chained pair of the split modes at C = 256 (kernels_conv_chain.hip, the ring form) against the two launches it replaces.

C4's identity pairs: P = branch2c (256 -> 1024, + residual, ReLU), Q = the next block's branch2a (1024 -> 256, ReLU).  The block's four
waves share a ring of two LDS stages that LDS-DMA fills from the layers' stream images (csrc/conv_pack.h), one block barrier per 64-column
chunk; a wave whose 32 rows lie beyond M keeps the ring going and does nothing else.  As for C = 64 / 128 (tests/test_gpu_conv_chain.py,
whose case maker, float64 reference and comparison this file uses) the launch is a policy, so both outputs and the watchdog word must agree
with conv_forward x 2 BIT FOR BIT, and the two launches themselves are held against float64.
"""
import functools
import importlib
import tempfile

import numpy as np
import pytest

import test_gpu_conv_chain as base

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")

C = 256
FP16_LIMIT = base.FP16_LIMIT
# B, H, W — M = 288: two full 128-row blocks and a ragged one, a tile across the image boundary; M = 64: half a block (waves 2 and 3 own no
# rows); M = 35: one full wave, a 3-row wave and two empty ones; M = 768: six blocks
CASES = [(2, 12, 12), (1, 8, 8), (1, 5, 7), (3, 16, 16)]


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    return base.make(C, B, H, W, False, seed=C + 7 * B + H)


@functools.lru_cache(maxsize=None)
def _two_launches(B, H, W, dtype, in_place):
    y, t1, flag = base.chain(_case(B, H, W), dtype, False, in_place)
    y.setflags(write=False); t1.setflags(write=False)
    return y, t1, flag


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("B,H,W", CASES)
def test_chained_equals_the_two_launches_bitwise(B, H, W, dtype, in_place):
    y0, t0, f0 = _two_launches(B, H, W, dtype, in_place)
    y1, t1, f1 = base.chain(_case(B, H, W), dtype, True, in_place)
    assert np.isfinite(y1).all() and np.isfinite(t1).all()
    assert (y0 == 0).mean() > 0.1 and (t0 == 0).mean() > 0.1 and (y0 > 0).mean() > 0.1 and (t0 > 0).mean() > 0.1      # ReLU cuts a good share of both
    base._same_bits(y1, y0, "y")
    base._same_bits(t1, t0, "t1")
    assert f1 == f0 == 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("B,H,W", CASES)
def test_the_two_launches_against_float64(B, H, W, dtype):
    y0, t0, _ = _two_launches(B, H, W, dtype, 0)
    ry, rt = base.ref64(_case(B, H, W), y0)
    tol = {"f32s": 2e-5, "f32x3": 1e-5}[dtype]          # tests/test_gpu_conv_kernels.py's bound for these modes
    ey, et = np.abs(y0 - ry).max(), np.abs(t0 - rt).max()
    print(f"C {C} B {B} {H}x{W} {dtype}: y err {ey:.3e} of max {np.abs(ry).max():.3e}, t1 err {et:.3e} of max {np.abs(rt).max():.3e}")
    assert ey <= tol * max(1.0, np.abs(ry).max()), (ey, np.abs(ry).max())
    assert et <= tol * max(1.0, np.abs(rt).max()), (et, np.abs(rt).max())


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_watchdog_words_agree(dtype):
    """the three plants of tests/test_gpu_conv_chain.py at C = 256"""
    b = _case(2, 12, 12)
    # a single y element past the fp16 range: one residual element (ragged last tile, second image)
    hot_y = dict(b)
    hot_y["x"] = b["x"].copy()
    hot_y["x"][1, 11, 5, 3 * C + 17] = 70000.0
    hot_y["s3"] = np.abs(b["s3"])
    # ... only in t1: one column's shift
    hot_t = dict(b)
    hot_t["h1"] = b["h1"].copy()
    hot_t["h1"][C - 3] = 70000.0
    # just below the limit in both
    warm = dict(hot_y)
    warm["x"] = b["x"].copy()
    warm["x"][1, 11, 5, 3 * C + 17] = 64000.0
    warm["h1"] = b["h1"].copy()
    warm["h1"][C - 3] = 60000.0
    warm["s1"] = b["s1"].copy()
    warm["s1"][C - 3] = 1e-3
    for case, want, name in ((hot_y, 1, "y"), (hot_t, 1, "t1"), (warm, 0, "below")):
        y0, t0, f0 = base.chain(case, dtype, False, 1)
        y1, t1, f1 = base.chain(case, dtype, True, 1)
        if name == "y":
            assert (np.abs(y0) >= FP16_LIMIT).sum() == 1
        if name == "t1":
            assert np.abs(y0).max() < FP16_LIMIT and np.abs(t0).max() >= FP16_LIMIT
        if name == "below":
            assert 60000.0 < np.abs(y0).max() < FP16_LIMIT and 59000.0 < np.abs(t0).max() < FP16_LIMIT
        base._same_bits(y1, y0, name + ": y")
        base._same_bits(t1, t0, name + ": t1")
        assert f0 == want and f1 == want, (name, f0, f1)


def test_an_entry_pair_is_refused_with_a_status():
    """C = 256 chains identity pairs only: the shortcut's operands with chained = 1 fail, nothing falls back"""
    rng = np.random.default_rng(5)
    c = base.make(C, 1, 4, 4, False, seed=3)
    c["x"] = None
    c["cs"], c["ss"] = 512, 2
    c["xs"] = base._acts(rng, (1, 8, 8, 512))
    c["ws"] = (rng.standard_normal((4 * C, 512)) * np.sqrt(2.0 / 512)).astype(np.float32)
    c["s_s"], c["h_s"] = base._bn(rng, 4 * C)
    with pytest.raises(L.MrcnnError):
        base.chain(c, "f32x3", True, 0)


def _image(w, q):
    w = np.ascontiguousarray(w, np.float32)
    img = np.empty(w.size, np.uint16)
    L.check(L.lib().mrcnn_test_chain_stream_image(w.ctypes.data, C, int(q), img.ctypes.data))
    return img


def _read_byte(q):
    """The byte of its image at which the kernel reads filter element (row n, channel k): chunk * 32 KB + the offset inside the LDS stage.
    P: W3 (1024 rows x 256 channels), chunk n // 64 = [K step k // 32][row n % 64][64 B]; Q: W1 (256 rows x 1024 channels), chunk k // 64 =
    [K step (k // 32) % 2][row n][64 B]; in both the 16-B piece c = (k // 8) % 4 of row r sits at piece position c ^ ((r >> 2) & 3)."""
    rows, K = (C, 4 * C) if q else (4 * C, C)
    n, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    if q:
        chunk, line, r = k // 64, ((k // 32) % 2) * C + n, n
    else:
        chunk, line, r = n // 64, (k // 32) * 64 + n % 64, n % 64
    return chunk * 32768 + line * 64 + ((((k // 8) % 4) ^ ((r >> 2) & 3)) << 4) + (k % 8) * 2


@pytest.mark.parametrize("q", [False, True])
def test_stream_images_hold_every_filter_value_where_the_kernel_reads_it(q):
    byte = _read_byte(q)
    rows, K = byte.shape
    assert np.array_equal(np.sort(byte.ravel()), np.arange(rows * K) * 2)          # the rule addresses every 2-byte slot exactly once
    # a random filter: the slot the kernel reads for (n, k) holds that element's fp16
    w = (np.random.default_rng(11 + q).standard_normal((rows, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    assert np.array_equal(_image(w, q)[byte // 2], w.astype(np.float16).view(np.uint16))
    # exactly once: two filters that spell an element's own index (idx % 512 and idx // 512, integers fp16 holds) name, slot by slot, the
    # element an image holds there — every index once, at its slot
    idx = np.arange(rows * K).reshape(rows, K)
    lo = _image((idx % 512).astype(np.float32), q).view(np.float16).astype(np.int64)
    hi = _image((idx // 512).astype(np.float32), q).view(np.float16).astype(np.int64)
    held = hi * 512 + lo
    assert np.array_equal(np.sort(held), np.arange(rows * K))
    assert np.array_equal(held[byte // 2], idx)


@pytest.mark.parametrize("mode", ["f32x3", "f32s"])
def test_in_the_model_the_chain_changes_launches_and_nothing_else(mode):
    """The small ResNet-50 of tests/test_gpu_conv_chain.py (256^2, batch 2) with "conv_chain4" 0 (two launches) and 2 (chained at every grid
    size): detections, masks and the C4 / C5 taps bit for bit, four conv launches fewer (C4: b->c, c->d, d->e, e->f; a->b is left out: the entry
    block's branch2c carries the shortcut), the same algorithmic flops in the backbone and over all classes — also with stored split exponents."""
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(256, 256, 3), num_classes=21, pre_nms_max_proposals=500, max_proposals=64, max_detections=16)
    d = tempfile.mkdtemp(prefix="mrcnn_chain4_")
    weights.save_synthetic_models(d, cfg, seed=0, forced_load=True)
    img = np.random.default_rng(0).integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
    got = {}
    try:
        for calib in (False, True):
            for knob in (0, 2):
                L.check(L.lib().mrcnn_debug_set(b"conv_chain4", knob))
                m = models.load_maskrcnn(d, max_batch=2, compute_dtype=mode)
                if calib:
                    m.calibrate_split(img)
                det, masks = m.predict(img)
                m.conv_profile_enable(True)
                m.predict(img)
                m.conv_profile_enable(False)
                tiles, groups = m.conv_profile(), m.conv_profile_groups()
                got[calib, knob] = (det.copy(), np.asarray(masks).copy(), [m.read_tensor(n, b).copy() for n in ("C4", "C5") for b in range(2)],
                                    sum(v[0] for v in tiles.values()), groups["backbone"][2], sum(v[2] for v in tiles.values()))
                del m
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_chain4", 1))
    for calib in (False, True):
        two, one = got[calib, 0], got[calib, 2]
        assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)), calib
        assert np.array_equal(one[1], two[1]), calib
        for a, b in zip(one[2], two[2]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), calib
        assert two[3] - one[3] == 4, (calib, two[3], one[3])
        assert one[4] == two[4] and one[5] == two[5], (calib, one[4:], two[4:])
