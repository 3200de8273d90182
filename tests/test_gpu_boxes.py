"""GPU parity of the box path (csrc/kernels_boxes.hip) outside the one shape a predict gives it: batches in one launch, more than 1024
regions and class ids beyond 1024, the bitonic anchors, the K edges — through mrcnn_test_proposals_batch / mrcnn_test_detections_batch
(include/maskrcnn_hip_test.h), which bind and stride the engine's routines as a predict does.  The cases and the oracle's expectations come from
tests/boxes_cases.py (their conditions are proved in tests/test_boxes_cases_host.py).  Integer and byte work, all-IEEE box arithmetic:
every comparison is bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import boxes_cases as K

pytestmark = pytest.mark.gpu
F = np.float32
L = importlib.import_module("mask-rcnn-coreml_amd._lib")
STD4 = np.asarray(K.STD, F)
MRCNN_ERR_UNSUPPORTED = 5


def _knob(name, value):
    L.check(L.lib().mrcnn_debug_set(name.encode(), value))


def run_proposals(images, anchors, pre_nms, max_proposals, nms_thr, row_stride=6):
    """images: [(probs, deltas)] -> (rois (B, max_proposals, row_stride) from a sentinel-filled buffer, keep_count (B))."""
    B, A = len(images), anchors.shape[0]
    probs = np.ascontiguousarray(np.stack([p for p, _ in images]), F)
    deltas = np.ascontiguousarray(np.stack([d for _, d in images]), F)
    anchors = np.ascontiguousarray(anchors, F)
    rois = np.full((B, max_proposals, row_stride), K.SENTINEL, F)
    count = np.full(B, -1, np.int32)
    L.check(L.lib().mrcnn_test_proposals_batch(probs.ctypes.data, deltas.ctypes.data, anchors.ctypes.data, B, A, STD4.ctypes.data, pre_nms, max_proposals,
                                               C.c_float(nms_thr), rois.ctypes.data, row_stride, count.ctypes.data))
    return rois, count


def run_detections(images, max_det, nms_thr=K.DET_NMS_THR, row_stride=6, score_thr=K.SCORE_THR):
    B, n = len(images), images[0][0].shape[0]
    rois = np.ascontiguousarray(np.stack([r for r, _ in images]), F)
    cls6 = np.ascontiguousarray(np.stack([c for _, c in images]), F)
    out = np.full((B, max_det, row_stride), K.SENTINEL, F)
    L.check(L.lib().mrcnn_test_detections_batch(rois.ctypes.data, cls6.ctypes.data, B, n, STD4.ctypes.data, max_det, C.c_float(score_thr), C.c_float(nms_thr),
                                                out.ctypes.data, row_stride))
    return out


def check_batch_alone_reversed(run, images, want):
    """Every image of the batch equals its oracle result, the same image sent alone, and its place in the reversed batch."""
    got = run(images)
    for b, w in enumerate(want):
        np.testing.assert_array_equal(got[b], w, err_msg=f"image {b} of the batch")
    for b in range(len(images)):
        np.testing.assert_array_equal(run([images[b]])[0], got[b], err_msg=f"image {b} alone")
    rev = run(images[::-1])
    np.testing.assert_array_equal(rev[::-1], got, err_msg="reversed batch")
    return got


# ------------------------------------------------------------------------------------------------
# proposals
# ------------------------------------------------------------------------------------------------
def test_proposals_batch_of_five():
    """{random, all-equal scores, ties across the selection threshold, long suppression chain, pairs on the IoU boundary} in one call;
    A = 4091 is odd (images 1 and 3: the scalar branch of the key kernel) and no multiple of 1024; row stride 6 over a sentinel."""
    a = K.proposal_anchors()
    images = [K.proposal_image(n) for n in K.PROPOSAL_IMAGES]
    want, counts = [], []
    for p, d in images:
        w, dbg = K.proposal_expect(p, d, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR, debug=True)
        want.append(w); counts.append(dbg["count"])
    run = lambda ims: run_proposals(ims, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR)[0]
    got = check_batch_alone_reversed(run, images, want)
    _, kc = run_proposals(images, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR)
    assert list(kc) == counts
    for b, n in enumerate(counts):                               # (implied by the oracle's buffer; spelled out)
        assert (got[b, :n, 4:] == K.SENTINEL).all() and (got[b, n:] == 0).all()


@pytest.mark.parametrize("pre_nms", [1, 63, 64, 65, 1024, 1025])
def test_proposals_k_edges(pre_nms):
    """K = preNMSMaxProposals around the steps of W = ceil(K / 64) and Kpad = next_pow2(K), both sort forms; B = 2."""
    a = K.proposal_anchors()
    images = [K.proposal_image("random"), K.proposal_image("ties")]
    want = [K.proposal_expect(p, d, a, pre_nms, K.PROP_MAXP, 0.7) for p, d in images]
    try:
        for rank in (1, 0):
            _knob("proposal_rank_sort", rank)
            got, _ = run_proposals(images, a, pre_nms, K.PROP_MAXP, 0.7)
            for b in range(2):
                np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b}, rank sort {rank}")
    finally:
        _knob("proposal_rank_sort", 1)


def test_proposals_tiny():
    """A = 5, preNMSMaxProposals = 3, maxProposals = 2."""
    a = K.random_anchors(5)
    images = [K.proposal_image("random", 5), K.proposal_image("ties", 5)]
    want = [K.proposal_expect(p, d, a, 3, 2, 0.7) for p, d in images]
    got, _ = run_proposals(images, a, 3, 2, 0.7)
    for b in range(2):
        np.testing.assert_array_equal(got[b], want[b])


@pytest.mark.parametrize("pre_nms", [300, 1000, 1500, 3000, 12000])
def test_bitonic_anchors_equal_rank_counting(pre_nms):
    """The one-block bitonic sorts — all-LDS (Kpad < 1024) and k_sort_decode<E> with E = 1, 2, 4, 16 — against rank counting and the oracle."""
    A = 16368
    a = K.random_anchors(A)
    images = [K.proposal_image("random", A), K.proposal_image("ties", A)]
    want = [K.proposal_expect(p, d, a, pre_nms, 100, 0.7, row_stride=4) for p, d in images]
    try:
        for rank in (0, 1):
            _knob("proposal_rank_sort", rank)
            got, _ = run_proposals(images, a, pre_nms, 100, 0.7, row_stride=4)
            for b in range(2):
                np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b}, rank sort {rank}")
    finally:
        _knob("proposal_rank_sort", 1)


def test_column_split_policy_across_batch_sizes():
    """K = 6000 (W = 94): the suppression-matrix grid has 24 column splits for one image and 5 for eight — the same bits."""
    A = 16368
    a = K.random_anchors(A)
    ties = K.proposal_image("ties", A)
    rng = np.random.default_rng(77)
    images = []
    for b in range(8):
        fg = rng.random(A, dtype=F)
        images.append((np.stack([1 - fg, fg], 1).astype(F), (0.5 * rng.standard_normal((A, 4))).astype(F)))
    images[3] = ties
    want = K.proposal_expect(*ties, a, 6000, 6000, 0.7, row_stride=4)
    alone, c1 = run_proposals([ties], a, 6000, 6000, 0.7, row_stride=4)
    batch, c8 = run_proposals(images, a, 6000, 6000, 0.7, row_stride=4)
    np.testing.assert_array_equal(alone[0], want)
    np.testing.assert_array_equal(batch[3], want)
    assert c1[0] == c8[3] and alone[0].tobytes() == batch[3].tobytes()
    for b in (0, 7):
        np.testing.assert_array_equal(batch[b], K.proposal_expect(*images[b], a, 6000, 6000, 0.7, row_stride=4), err_msg=f"image {b}")


# ------------------------------------------------------------------------------------------------
# detections
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [1, 0])
def test_detections_batch_of_four(fast):
    """{nothing passes, everything passes in 3 saturating classes, 81 random classes with equal-score runs, all boxes identical}, N = 1000;
    row stride 8 over a sentinel."""
    images = [K.detection_image(n) for n in K.DETECTION_IMAGES]
    want = [K.detection_expect(r, c, 100, row_stride=8) for r, c in images]
    try:
        _knob("nms_class_fast", fast)
        check_batch_alone_reversed(lambda ims: run_detections(ims, 100, row_stride=8), images, want)
    finally:
        _knob("nms_class_fast", 1)


@pytest.mark.parametrize("n", [1024, 1025, 2500, 8192])
def test_detections_beyond_1024_regions(n):
    """More than one pass of the filter's 1024-wide loop, Npad >= 2048 in the final sort, more than 16 column words per matrix row; 8192 = the limit."""
    images = [K.detection_image("many", n), K.detection_image("sparse", n)]
    want = [K.detection_expect(r, c, 100) for r, c in images]
    got = run_detections(images, 100)
    for b in range(2):
        np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b}")


def test_detection_layer_2500_regions(pkg):
    """The same N = 2500 image through DetectionLayer.evaluate."""
    rois, c = K.detection_image("many", 2500)
    layer = pkg.DetectionLayer({"maxDetections": 100, "scoreThreshold": K.SCORE_THR, "nmsIOUThreshold": K.DET_NMS_THR})
    ML = pkg.MLMultiArray
    out = np.full((100, 6), np.float32(np.nan), dtype=F)
    layer.evaluate([ML(np.array(rois)), ML(np.array(c))], [ML(out)])
    np.testing.assert_array_equal(out, K.detection_expect(rois, c, 100))


def test_detections_8193_regions_are_refused():
    images = [K.detection_image("sparse", 8193)] * 2
    rois = np.ascontiguousarray(np.stack([r for r, _ in images]), F)
    cls6 = np.ascontiguousarray(np.stack([c for _, c in images]), F)
    out = np.full((2, 100, 6), K.SENTINEL, F)
    st = L.lib().mrcnn_test_detections_batch(rois.ctypes.data, cls6.ctypes.data, 2, 8193, STD4.ctypes.data, 100, C.c_float(K.SCORE_THR),
                                             C.c_float(K.DET_NMS_THR), out.ctypes.data, 6)
    assert st == MRCNN_ERR_UNSUPPORTED, L.lib().mrcnn_last_error()
    assert (out == K.SENTINEL).all()


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("max_det", [7, 80])
@pytest.mark.parametrize("n", [1000, 2500])
def test_detections_large_class_ids(n, max_det, fast):
    """Class ids 1019 .. 1030: ids >= 1024 are counted from kept_cls[] by the ballot loop (more than one round at max_det = 80), chunks mix
    them with table-counted ids, and a large id reaches the limit inside a chunk.  B = 2: the case and the N > 1024 image side by side."""
    images = [K.detection_image("large_ids", n), K.detection_image("many", n)]
    want = [K.detection_expect(r, c, max_det) for r, c in images]
    try:
        _knob("nms_class_fast", fast)
        got = run_detections(images, max_det)
    finally:
        _knob("nms_class_fast", 1)
    for b in range(2):
        np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b}")


def test_bad_arguments_return_a_status():
    z = np.zeros(64, F)
    p = z.ctypes.data
    lib = L.lib()
    assert lib.mrcnn_test_proposals_batch(p, p, p, 0, 4, STD4.ctypes.data, 4, 2, C.c_float(0.7), p, 4, None) != 0        # batch 0
    assert lib.mrcnn_test_proposals_batch(p, p, p, 1, 4, STD4.ctypes.data, 4, 2, C.c_float(0.7), p, 3, None) != 0        # row stride < 4
    assert lib.mrcnn_test_proposals_batch(None, p, p, 1, 4, STD4.ctypes.data, 4, 2, C.c_float(0.7), p, 4, None) != 0
    assert lib.mrcnn_test_detections_batch(p, p, 1, 4, STD4.ctypes.data, 2, C.c_float(0.7), C.c_float(0.3), p, 5) != 0    # row stride < 6
    assert lib.mrcnn_test_detections_batch(p, p, 1, 0, STD4.ctypes.data, 2, C.c_float(0.7), C.c_float(0.3), p, 6) != 0    # no regions
    assert (z == 0).all()


# ------------------------------------------------------------------------------------------------
# a caller-supplied nmsIOUThreshold < 0: IOU() >= 0 > thr for every pair — only the first selectable box (per class) survives
# ------------------------------------------------------------------------------------------------
def test_negative_nms_threshold():
    a = K.random_anchors(150).copy()
    p, d = K.proposal_image("random", 150)
    d = np.zeros_like(d)
    a[int(np.argmax(p[:, 1])), 2] = a[int(np.argmax(p[:, 1])), 0]          # the best-scoring box has no height: not selectable
    images = [(p, d), K.proposal_image("ties", 150)]
    got, kc = run_proposals(images, a, 150, 50, -1.0)
    for b in range(2):
        np.testing.assert_array_equal(got[b], K.proposal_expect(*images[b], a, 150, 50, -1.0), err_msg=f"image {b}")
    assert list(kc) == [1, 1]
    dets = [K.detection_image("random81", 200), K.detection_image("identical", 200)]
    got = run_detections(dets, 100, nms_thr=-1.0)
    for b in range(2):
        np.testing.assert_array_equal(got[b], K.detection_expect(*dets[b], 100, nms_thr=-1.0), err_msg=f"image {b}")
