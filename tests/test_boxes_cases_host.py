"""The box-path cases (tests/boxes_cases.py) are what they claim — proved from the CPU oracle alone, no GPU: the conditions that send
csrc/kernels_boxes.hip down its rarely taken branches hold by the reference, not by the code under test (tests/test_gpu_boxes.py)."""
import numpy as np
import pytest

import boxes_cases as K

F = np.float32


def test_chain_image_is_a_long_chain_and_sparse():
    """keep, drop, keep ... over the first 40 candidates, then runs in which one kept box suppresses dozens: fewer keeps than maxProposals,
    so zero padding is written; the candidates are the chain anchors in index order and decode to themselves."""
    a = K.proposal_anchors()
    p, d = K.proposal_image("chain")
    out, dbg = K.proposal_expect(p, d, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR, debug=True)
    assert list(dbg["topk_idx"]) == list(range(K.N_CHAIN)) and K.N_CHAIN == K.PROP_PRE
    assert list(dbg["keep"][:K.N_ALT // 2]) == list(range(0, K.N_ALT, 2))
    assert K.N_ALT // 2 + K.N_DENSE_ROWS <= dbg["count"] < K.PROP_MAXP
    gaps = np.diff(dbg["keep"][K.N_ALT // 2:])
    assert gaps.max() > 30                                       # one kept box answers for more than 30 later rows
    assert (out[dbg["count"]:] == 0).all() and (out[:dbg["count"], 4:] == K.SENTINEL).all()


def test_pairs_image_sits_on_the_threshold():
    a = K.proposal_anchors()
    p, d = K.proposal_image("pairs")
    _, dbg = K.proposal_expect(p, d, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR, debug=True)
    n2 = 2 * K.N_PAIRS
    assert list(dbg["topk_idx"][:n2]) == list(range(K.PAIR0, K.PAIR0 + n2))
    np.testing.assert_array_equal(dbg["boxes"][:n2], a[K.PAIR0:K.PAIR0 + n2])             # zero deltas on dyadic boxes: exact
    kept = set(int(k) for k in dbg["keep"])
    kinds = {0: [], 1: [], 2: []}
    for k in range(K.N_PAIRS):
        f = F(K.orc.iou(dbg["boxes"][2 * k + 1], dbg["boxes"][2 * k]))
        kinds[k % 3].append((f, (2 * k + 1) in kept, (2 * k) in kept))
    assert all(f == K.PAIR_THR and partner and first for f, partner, first in kinds[0])    # IoU == thr: not above, kept
    assert all(f > K.PAIR_THR and not partner and first for f, partner, first in kinds[1])
    assert all(f < K.PAIR_THR and partner and first for f, partner, first in kinds[2])
    assert all(abs(float(f) - float(K.PAIR_THR)) < 1e-4 for v in kinds.values() for f, _, _ in v)
    assert dbg["count"] == K.PROP_MAXP                           # ... and the image fills its 64 rows


@pytest.mark.parametrize("name", ["ties", "all_equal"])
def test_more_anchors_tie_at_the_kth_score_than_the_selection_takes(name):
    p, _ = K.proposal_image(name)
    for pre in (63, 64, 65, K.PROP_PRE, 1024, 1025):
        ngt, nties, need = K.tie_stats(p, pre)
        assert 1 <= need < nties, (pre, ngt, nties, need)
    p, _ = K.proposal_image(name, 16368)
    for pre in (300, 1000, 1500, 3000, 12000):
        ngt, nties, need = K.tie_stats(p, pre)
        assert 1 <= need < nties, (pre, ngt, nties, need)


def test_all_equal_image_is_sparse_too():
    a = K.proposal_anchors()
    p, d = K.proposal_image("all_equal")
    _, dbg = K.proposal_expect(p, d, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR, debug=True)
    assert list(dbg["topk_idx"]) == list(range(K.PROP_PRE)) and dbg["count"] < K.PROP_MAXP


def test_random_image_fills_its_rows_early():
    a = K.proposal_anchors()
    p, d = K.proposal_image("random")
    _, dbg = K.proposal_expect(p, d, a, K.PROP_PRE, K.PROP_MAXP, K.PAIR_THR, debug=True)
    assert dbg["count"] == K.PROP_MAXP and dbg["keep"][-1] < K.PROP_PRE - 64          # the scan stops chunks before the end


def test_column_split_image_scans_every_chunk():
    """pre_nms 6000 of 16368 random anchors with room for every candidate (maxProposals 6000): hundreds are suppressed and the scan runs to
    the last chunk — it reads every column word of the suppression matrix, whichever split computed it."""
    a = K.random_anchors(16368)
    for name in ("ties", "random"):
        p, d = K.proposal_image(name, 16368)
        _, dbg = K.proposal_expect(p, d, a, 6000, 6000, 0.7, row_stride=4, debug=True)
        assert 3000 < dbg["count"] < 5500 and dbg["keep"][-1] >= 6000 - 64


def test_saturating_image_saturates_inside_a_chunk():
    rois, c = K.detection_image("saturating")
    tr = K.detection_trace(rois, c, 100)
    assert len(tr["src"]) == 1000                                # everything passes
    full = [k for k, v in tr["keeps"].items() if len(v) == 100 and len(tr["free"][k]) > 100]
    assert len(full) >= 2
    assert any(K.saturates_inside_a_chunk(tr, k, 100) for k in full)
    # ... and the other detection images: nothing passes | one keep per class | equal-score runs among the detections
    assert len(K.detection_trace(*K.detection_image("nothing"), 100)["src"]) == 0
    tr = K.detection_trace(*K.detection_image("identical"), 100)
    assert sorted(tr["keeps"]) == [1, 2, 3, 4, 5] and all(len(v) == 1 and v[0] == np.nonzero(tr["cls"] == k)[0][0] for k, v in tr["keeps"].items())
    want = K.detection_expect(*K.detection_image("random81"), 100)
    assert (np.diff(want[:, 5]) == 0).sum() >= 5 and want[-1, 5] > 0


@pytest.mark.parametrize("n", [1024, 1025, 2500, 8192])
@pytest.mark.parametrize("name", ["many", "sparse"])
def test_detections_beyond_1024_regions(name, n):
    rois, c = K.detection_image(name, n)
    tr = K.detection_trace(rois, c, 100)
    src = tr["src"]
    assert (src < 1024).any() and src[-1] == n - 1
    if n > 1024:
        assert (src >= 1024).any()
    if n > 2048:
        assert (src >= 2048).any()
    assert sum(len(v) for v in tr["keeps"].values()) > 100       # more NMS keeps than max_det: the final top-k cuts
    if name == "many" and n >= 2500:
        assert len(src) > 1024                                   # more than 16 column words per row of the suppression matrix


@pytest.mark.parametrize("n", [1000, 2500])
@pytest.mark.parametrize("max_det", [7, 80])
def test_large_id_cases(n, max_det):
    rois, c = K.detection_image("large_ids", n)
    tr = K.detection_trace(rois, c, max_det)
    cls = tr["cls"]
    assert cls.min() < 1024 <= cls.max() and set(np.unique(cls)) <= set(range(1019, 1031))
    # a chunk holds small and large ids side by side, both among the rows the scan keeps
    kept_pos = np.sort(np.concatenate(list(tr["keeps"].values())))
    mixed = [ch for ch in range(len(cls) // 64) if {bool(cls[q] >= 1024) for q in kept_pos[(kept_pos // 64) == ch]} == {True, False}]
    assert mixed
    big_full = [k for k, v in tr["keeps"].items() if k >= 1024 and len(v) == max_det and len(tr["free"][k]) > max_det]
    assert big_full                                              # a class beyond the counter table reaches the limit
    assert any(K.saturates_inside_a_chunk(tr, k, max_det) for k in big_full)
    if max_det >= 80:
        # every keep before the chunk where that class saturates sits in kept_cls[]: more than 64 of them, so the ballot loop runs a second round
        k = max(big_full, key=lambda k: len(tr["free"][k]))
        sat_chunk = int(tr["keeps"][k][max_det - 1]) // 64
        assert int((kept_pos < sat_chunk * 64).sum()) > 64
        assert int((tr["keeps"][k] < sat_chunk * 64).sum()) > 64


def test_negative_threshold_keeps_the_first_selectable_box():
    a = K.random_anchors(150).copy()
    p, d = K.proposal_image("random", 150)
    d = np.zeros_like(d)
    first = int(np.argmax(p[:, 1]))
    a[first, 2] = a[first, 0]                                    # the best-scoring box has no height: not selectable
    out, dbg = K.proposal_expect(p, d, a, 150, 50, -1.0, debug=True)
    assert dbg["count"] == 1 and dbg["keep"][0] == 1 and dbg["topk_idx"][0] == first
    rois, c = K.detection_image("random81", 200)
    tr = K.detection_trace(rois, c, 100, nms_thr=-1.0)
    assert len(tr["keeps"]) > 5 and all(len(v) == 1 for v in tr["keeps"].values())
