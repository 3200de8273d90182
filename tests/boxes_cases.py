"""Case makers of the box-path tests (csrc/kernels_boxes.hip): per-image inputs and the expectation from the CPU oracle, one image at a time.

No GPU and no HIP library here.  tests/test_boxes_cases_host.py proves from the oracle alone that every case is what it claims (a class
saturates inside a 64-row chunk, more anchors tie at the K-th score than the selection takes, ...); tests/test_gpu_boxes.py sends the same
cases through mrcnn_test_proposals_batch / mrcnn_test_detections_batch and compares bit for bit.  Everything is seeded: the two files see the
same arrays.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as orc

STD = (0.1, 0.1, 0.2, 0.2)
SENTINEL = np.float32(7.0)
F = np.float32

# ------------------------------------------------------------------------------------------------
# proposals
# ------------------------------------------------------------------------------------------------
PROP_A, PROP_PRE, PROP_MAXP = 4091, 1000, 64        # A odd: the probs rows of images 1 and 3 of a batch are 8-byte aligned only
N_ALT, N_DENSE_ROWS, N_DENSE = 40, 10, 96           # the chain anchors: indices [0, 1000)
N_CHAIN = N_ALT + N_DENSE_ROWS * N_DENSE
N_PAIRS = 30                                        # the boundary pairs: indices [1000, 1060), box then partner
PAIR0 = N_CHAIN
U = 2.0 ** -10                                      # the pairs' coordinates are multiples of 2^-10 (2^-20): exact in fp32 and fp64
PAIR_THR = F(53.0 / 75.0)                           # = Float(IoU) of two 64 x 64 boxes 11 units apart: THE threshold of the proposal batch


def _random_boxes(rng, n):
    y1 = rng.random(n) * 0.8
    x1 = rng.random(n) * 0.8
    h = 0.03 + rng.random(n) ** 2 * 0.4
    w = 0.03 + rng.random(n) ** 2 * 0.4
    return np.stack([y1, x1, np.minimum(y1 + h, 1.0), np.minimum(x1 + w, 1.0)], 1).astype(F)


@functools.lru_cache(maxsize=None)
def proposal_anchors():
    """(4091, 4).  [0, 40): a row of boxes each overlapping only its neighbours above the threshold (IoU 7/9 next, 6/10 the one after): keep,
    drop, keep ...; [40, 1000): ten rows of 96 boxes 1/200 of a width apart — one kept box suppresses the next ~34; [1000, 1060): 30 isolated
    pairs on a dyadic grid, IoU exactly on / a hair above / a hair below PAIR_THR; the rest random."""
    rng = np.random.default_rng(1001)
    a = _random_boxes(rng, PROP_A)
    for i in range(N_ALT):
        x1 = 0.01 + i * 0.02
        a[i] = [0.02, x1, 0.08, x1 + 0.16]
    for r in range(N_DENSE_ROWS):
        for i in range(N_DENSE):
            y1, x1 = 0.1 + 0.085 * r, 0.05 + i * 0.001
            a[N_ALT + r * N_DENSE + i] = [y1, x1, y1 + 0.08, x1 + 0.2]
    for k in range(N_PAIRS):
        oy, ox = (k // 6) * 160 + 8, (k % 6) * 160 + 8
        dx = 11.0 + (0.0, -2.0 ** -10, 2.0 ** -10)[k % 3]          # on the threshold | more overlap | less
        a[PAIR0 + 2 * k] = [oy * U, ox * U, (oy + 64) * U, (ox + 64) * U]
        a[PAIR0 + 2 * k + 1] = [oy * U, (ox + dx) * U, (oy + 64) * U, (ox + dx + 64) * U]
    a.setflags(write=False)
    return a


def _probs(fg):
    fg = np.asarray(fg, F)
    return np.stack([F(1) - fg, fg], axis=1).astype(F)


PROPOSAL_IMAGES = ("random", "all_equal", "ties", "chain", "pairs")


@functools.lru_cache(maxsize=None)
def proposal_image(name, A=PROP_A):
    """(probs (A,2), deltas (A,4)) of one image over proposal_anchors() (A = 4091) or random_anchors(A)."""
    rng = np.random.default_rng(2000 + sum(map(ord, name)) + A)
    if name == "random":
        fg, deltas = rng.random(A, dtype=F), (0.5 * rng.standard_normal((A, 4))).astype(F)
    elif name == "all_equal":
        fg, deltas = np.full(A, 0.5, F), np.zeros((A, 4), F)
    elif name == "ties":                 # 9 distinct scores: hundreds of anchors tie at the K-th
        fg, deltas = (np.round(rng.random(A) * 8) / 8).astype(F), (0.1 * rng.standard_normal((A, 4))).astype(F)
    elif name == "chain":                # the chain anchors first, in index order; everything else far behind
        fg = (0.3 * rng.random(A)).astype(F)
        fg[:N_CHAIN] = np.linspace(0.99, 0.6, N_CHAIN).astype(F)
        deltas = np.zeros((A, 4), F)
    elif name == "pairs":                # the pairs first (a box outranks its partner), then the rest: nothing ranked earlier can suppress a pair
        fg = (0.3 * rng.random(A)).astype(F)
        fg[PAIR0:PAIR0 + 2 * N_PAIRS] = np.linspace(0.99, 0.6, 2 * N_PAIRS).astype(F)
        deltas = (0.3 * rng.standard_normal((A, 4))).astype(F)
        deltas[PAIR0:PAIR0 + 2 * N_PAIRS] = 0
    else:
        raise KeyError(name)
    p = _probs(fg)
    p.setflags(write=False); deltas.setflags(write=False)
    return p, deltas


@functools.lru_cache(maxsize=None)
def random_anchors(A, seed=1002):
    a = _random_boxes(np.random.default_rng(seed + A), A)
    a.setflags(write=False)
    return a


def proposal_expect(probs, deltas, anchors, pre_nms, max_proposals, nms_thr, row_stride=6, debug=False):
    """The oracle's rois for one image in a sentinel-filled (max_proposals, row_stride) buffer: kept rows carry 4 coordinates and the
    sentinel behind them, padded rows are zero throughout (ProposalLayer.swift:178-192)."""
    out = np.full((max_proposals, row_stride), SENTINEL, F)
    return orc.proposal_layer(probs, deltas, anchors, pre_nms, max_proposals, float(nms_thr), out_stride=row_stride, out=out, debug=debug)


def tie_stats(probs, K):
    """(anchors scoring above the K-th score, anchors tying with it, how many of those the selection takes = ST_NEED)."""
    s = np.sort(probs[:, 1])[::-1]
    t = s[K - 1]
    ngt, nties = int((probs[:, 1] > t).sum()), int((probs[:, 1] == t).sum())
    return ngt, nties, K - ngt


# ------------------------------------------------------------------------------------------------
# detections
# ------------------------------------------------------------------------------------------------
SCORE_THR, DET_NMS_THR = 0.7, 0.3


def _small_rois(rng, n, big_frac=0.0):
    y1 = rng.random(n) * 0.9
    x1 = rng.random(n) * 0.9
    wh = np.where(rng.random(n) < big_frac, 0.15, 0.02)
    return np.stack([y1, x1, y1 + wh, x1 + wh * (0.5 + rng.random(n))], 1).astype(F)


def _cls6(rng, n, ids, p=None, pass_frac=1.0, delta_scale=0.1):
    c = np.zeros((n, 6), F)
    c[:, :4] = (delta_scale * rng.standard_normal((n, 4))).astype(F)
    c[:, 4] = rng.choice(np.asarray(ids), n, p=p).astype(F)
    s = rng.random(n)
    c[:, 5] = np.where(rng.random(n) < pass_frac, 0.7 + 0.3 * s, 0.69 * s).astype(F)
    return c


DETECTION_IMAGES = ("nothing", "saturating", "random81", "identical")


@functools.lru_cache(maxsize=None)
def detection_image(name, n=1000):
    """(rois (n,4), cls6 (n,6))."""
    rng = np.random.default_rng(3000 + sum(map(ord, name)) + n)
    if name == "nothing":
        rois, c = _small_rois(rng, n, 0.5), _cls6(rng, n, range(0, 81), pass_frac=0.0)
    elif name == "saturating":           # everything passes, three classes of mostly disjoint boxes: each reaches max_det a third of the way in
        rois, c = _small_rois(rng, n, 0.1), _cls6(rng, n, (1, 2, 3))
    elif name == "random81":
        rois, c = _small_rois(rng, n, 0.5), _cls6(rng, n, range(0, 81), pass_frac=0.6, delta_scale=1.0)
        c[3, 5] = 0.7                                            # exactly at the threshold: kept
        c[4, 5] = np.nextafter(F(0.7), F(0))                     # just below: dropped
        rois[10] = 0                                             # zero area: never selected
        for lo in range(20, n - 40, 97):                         # runs of equal scores across classes: the stable order decides
            c[lo:lo + 30, 5] = F(0.96) + F(0.001) * F(lo % 7)
    elif name == "identical":            # one box, n times: a class keeps its first row only
        rois = np.tile(np.asarray([[0.2, 0.3, 0.6, 0.7]], F), (n, 1))
        c = _cls6(rng, n, (1, 2, 3, 4, 5), pass_frac=0.8, delta_scale=0.0)
    elif name == "many":                 # N > 1024: most rows pass, 20 classes of small boxes — far more keeps than max_det
        rois, c = _small_rois(rng, n, 0.3), _cls6(rng, n, range(0, 21), pass_frac=0.8)
        c[n - 1, 4:] = (3.0, 0.999)                              # the last row passes, whatever n
    elif name == "sparse":               # N > 1024: one row in five passes
        rois, c = _small_rois(rng, n, 0.3), _cls6(rng, n, range(0, 21), pass_frac=0.2)
        c[n - 1, 4:] = (3.0, 0.999)
    elif name == "large_ids":            # ids straddling the 1024-entry counter table; 1027 holds 40 % of the rows, 1021 a quarter
        ids = np.arange(1019, 1031)
        p = np.full(12, 0.35 / 10)
        p[1027 - 1019], p[1021 - 1019] = 0.40, 0.25
        rois, c = _small_rois(rng, n, 0.15), _cls6(rng, n, ids, p=p)
    else:
        raise KeyError(name)
    rois.setflags(write=False); c.setflags(write=False)
    return rois, c


def detection_expect(rois, cls6, max_det, row_stride=6, score_thr=SCORE_THR, nms_thr=DET_NMS_THR):
    """The oracle's detections for one image in a sentinel-filled (max_det, row_stride) buffer: detection rows carry six values and the
    sentinel behind them, padded rows are zero throughout (DetectionLayer.swift:211-231)."""
    want, nd = orc.detection_layer(rois, cls6, max_det, score_thr, nms_thr, return_count=True)
    out = np.full((max_det, row_stride), SENTINEL, F)
    out[:, :6] = want
    out[nd:] = 0
    return out


def detection_trace(rois, cls6, max_det, score_thr=SCORE_THR, nms_thr=DET_NMS_THR):
    """What the oracle's pieces say happens inside DetectionLayer.evaluate, for the case conditions: src = the rows passing the filter
    (DetectionLayer.swift:238-276, :136-140), cls = their class ids, keeps[c] = positions (in the filtered order) the per-class
    nonMaxSupression call selects (at most max_det), free[c] = the same without a limit."""
    s, cid = cls6[:, 5], cls6[:, 4]
    src = np.nonzero((np.where(s >= F(score_thr), s, F(0)) != 0) & (cid > 0))[0]
    d = (cls6[src, :4] * np.asarray(STD, F)).astype(F)
    boxes = orc.clip_boxes(orc.apply_box_deltas(rois[src], d)) if src.size else np.zeros((0, 4), F)
    cls = cid[src].astype(np.int64)
    keeps, free = {}, {}
    for c in np.unique(cls):
        idx = np.nonzero(cls == c)[0]
        keeps[int(c)] = orc.nms(boxes, idx, nms_thr, max_det)
        free[int(c)] = orc.nms(boxes, idx, nms_thr, len(idx))
    return {"src": src, "cls": cls, "boxes": boxes, "keeps": keeps, "free": free}


def saturates_inside_a_chunk(tr, c, max_det):
    """Class c takes its max_det-th keep at a position of the filtered order behind which, in the same 64-row chunk, a row of the class
    follows that an unlimited scan keeps: the limit alone refuses it."""
    k = tr["keeps"][c]
    if len(k) < max_det:
        return False
    last = int(k[max_det - 1])
    later = [int(q) for q in tr["free"][c] if q > last and q // 64 == last // 64]
    return bool(later)
