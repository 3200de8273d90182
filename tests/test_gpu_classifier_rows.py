"""k_softmax_rows + k_classifier_post on caller rows (mrcnn_classifier_rows): the classifier head behind its last inner product.

Through whole layers the two kernels only ever met finite rows at nc in {2, 3, 5, 21, 81}.  Here: class counts on both sides of the
64-lane wave (one lane per class, then a second trip of the lanes' loop), a padded row stride whose padding is poisoned, logits far
apart, exact ties — and the rows a LOCAL fp16-range overflow hands these kernels before the watchdog word is read: one +Inf logit,
one NaN logit, all -Inf.  Each of those makes every probability of the row NaN (inf - inf), and the arg-max must still index inside
the row: class 0, the NaN as the score, class 0's deltas (oracle/mrcnn_oracle.c: orc_classifier_postprocess), a row DetectionLayer drops.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")

PROB_CEILING = 2e-5          # the project's absolute ceiling for probabilities (tests/test_gpu_fp64_stages.py::_ceiling)
NCS = [1, 2, 63, 64, 65, 81, 129]


def classifier_rows(logits, bbox, nc):
    n, ld = logits.shape
    lg = np.ascontiguousarray(logits, np.float32)
    bb = np.ascontiguousarray(bbox, np.float32)
    probs = np.full((n, nc), np.float32(7.0), np.float32)
    cls6 = np.full((n, 6), np.float32(7.0), np.float32)
    L.check(L.lib().mrcnn_classifier_rows(lg.ctypes.data, ld, bb.ctypes.data, nc, n, probs.ctypes.data, cls6.ctypes.data))
    return probs, cls6


def softmax64(logits):
    """Row softmax in float64, the maximum subtracted.  Rows without a finite maximum, or with a NaN, come out NaN as a whole —
    the same arithmetic in any precision: inf - inf, or a NaN term in the sum."""
    x = logits.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - np.max(x, axis=1, keepdims=True))          # np.max propagates NaN: the whole row turns NaN
        return e / e.sum(axis=1, keepdims=True)


def _finite_rows(nc, rng):
    """Logit rows (name, row) whose softmax is finite."""
    rows = [("normal", rng.standard_normal(nc) * 3) for _ in range(9)]          # 9 rows: more than two blocks of four waves, the last ragged
    rows.append(("pm80", rng.choice([-80.0, 80.0], nc)))
    rows.append(("pm1e4", rng.choice([-1e4, 1e4], nc)))
    one_hi = np.full(nc, -1e4); one_hi[nc - 1] = 1e4                            # the only large entry in the last column
    rows.append(("last_column", one_hi))
    rows.append(("one_minus_inf", np.where(np.arange(nc) == nc // 2, -np.inf if nc > 1 else 0.0, rng.standard_normal(nc))))
    return rows


def _tie_rows(nc, rng):
    """(row, class that must win): bit-equal maxima -> the lowest index."""
    out = [(np.full(nc, 1.25), 0)]
    if nc >= 3:
        r = rng.standard_normal(nc) - 10.0
        r[[1, nc - 1]] = 3.5                                                     # first and last lane trip
        out.append((r, 1))
    if nc > 64:
        r = rng.standard_normal(nc) - 10.0
        r[[nc - 1, 64, 63]] = 2.0                                                # lane 0's second trip ties with lane 63's first
        out.append((r, 63))
        r = rng.standard_normal(nc) - 10.0
        r[[64, 5]] = 2.0                                                         # one lane sees the higher index first
        out.append((r, 5))
    return out


def _nonfinite_rows(nc, rng):
    out = []
    for pos in sorted({0, nc // 2, nc - 1}):
        for bad in (np.inf, np.nan):
            r = rng.standard_normal(nc)
            r[pos] = bad
            out.append(r)
    out.append(np.full(nc, -np.inf))
    r = rng.standard_normal(nc)
    r[0] = np.inf; r[nc - 1] = np.nan
    out.append(r)
    return out


@pytest.mark.parametrize("nc", NCS)
def test_classifier_rows_against_float64(nc, orc):
    rng = np.random.default_rng(1000 + nc)
    finite = _finite_rows(nc, rng)
    ties = _tie_rows(nc, rng)
    nonfin = _nonfinite_rows(nc, rng)
    rows = [r for _, r in finite] + [r for r, _ in ties] + nonfin
    n, ld = len(rows), nc + 3
    logits = np.full((n, ld), np.nan, np.float32)          # the padding is poison: a read past nc turns a finite row NaN
    logits[:, :nc] = np.asarray(rows, np.float32)
    # interleave: a non-finite row shares its block of four waves with finite ones
    perm = rng.permutation(n)
    logits = logits[perm]
    kind = np.array(["finite"] * len(finite) + ["tie"] * len(ties) + ["nonfinite"] * len(nonfin))[perm]
    tie_winner = np.array([-1] * len(finite) + [w for _, w in ties] + [-1] * len(nonfin))[perm]
    bbox = rng.standard_normal((n, nc * 4)).astype(np.float32)

    probs, cls6 = classifier_rows(logits, bbox, nc)
    ref = softmax64(logits[:, :nc])
    fin = kind != "nonfinite"
    assert np.isfinite(ref[fin]).all() and np.isnan(ref[~fin]).all()          # the cases are what their names say

    # probabilities
    err = np.abs(probs[fin].astype(np.float64) - ref[fin]).max()
    print(f"nc {nc}: max |p - p64| = {err:.3g}")
    assert err <= PROB_CEILING
    assert np.isnan(probs[~fin]).all()

    # class id: exact wherever float64 separates the top two by more than the ceiling
    ids = cls6[:, 4].astype(np.int64)
    assert ((ids >= 0) & (ids < nc)).all()
    top = np.sort(ref[fin], axis=1)
    gap = top[:, -1] - top[:, -2] if nc > 1 else np.ones(fin.sum())
    decided = gap > PROB_CEILING
    assert decided.sum() >= 9                                                   # the random rows at least
    np.testing.assert_array_equal(ids[fin][decided], np.argmax(ref[fin], axis=1)[decided])
    t = kind == "tie"
    np.testing.assert_array_equal(ids[t], tie_winner[t])

    # the whole record, bit for bit, on the GPU's own probabilities (finite rows) and as defined (non-finite rows)
    np.testing.assert_array_equal(cls6, orc.classifier_postprocess(probs, bbox))
    want = orc.classifier_postprocess(ref, bbox)[~fin]
    np.testing.assert_array_equal(want[:, 4], 0)
    assert np.isnan(want[:, 5]).all()
    np.testing.assert_array_equal(want[:, :4], bbox[~fin, :4])
    np.testing.assert_array_equal(cls6[~fin], want)
    np.testing.assert_array_equal(cls6[:, 5][fin], probs[fin][np.arange(fin.sum()), ids[fin]])


def test_detection_layer_drops_the_rows_without_a_comparable_entry(pkg, orc):
    """What the definition promises downstream: records with a NaN score (class 0) never become detections, on the GPU and in the
    oracle alike, and the finite rows around them are treated as if they were not there."""
    nc, n, maxd = 21, 40, 16
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((n, nc)) * 6).astype(np.float32)
    bad = np.array([0, 7, 8, 39])
    logits[0, 3] = np.inf; logits[7, 0] = np.nan; logits[8, :] = -np.inf; logits[39, nc - 1] = np.inf
    bbox = (0.1 * rng.standard_normal((n, nc * 4))).astype(np.float32)
    _, cls6 = classifier_rows(logits, bbox, nc)
    assert np.isnan(cls6[bad, 5]).all() and (cls6[bad, 4] == 0).all()
    y1 = rng.random(n) * 0.8; x1 = rng.random(n) * 0.8
    rois = np.stack([y1, x1, y1 + 0.1, x1 + 0.15], 1).astype(np.float32)
    ML = pkg.MLMultiArray
    out = np.full((maxd, 6), np.float32(np.nan), dtype=np.float32)
    pkg.DetectionLayer({"maxDetections": maxd, "scoreThreshold": 0.7, "nmsIOUThreshold": 0.3}).evaluate([ML(rois), ML(cls6)], [ML(out)])
    want = orc.detection_layer(rois, cls6, maxd, 0.7, 0.3)
    np.testing.assert_array_equal(out, want)
    assert np.isfinite(out).all() and (out[:, 5] > 0).any()
    good = np.setdiff1d(np.arange(n), bad)
    np.testing.assert_array_equal(out, orc.detection_layer(rois[good], cls6[good], maxd, 0.7, 0.3))
