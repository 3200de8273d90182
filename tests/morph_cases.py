"""The cases of the morphology tests (tests/test_rle_morph_host.py, tests/test_gpu_rle_morph.py) and a numpy restatement of the rule of
include/maskrcnn_hip.h on dense planes: zero padding and a window of shifted slices.

Planes: 1x1, 1x7, 7x1, 5x5; sides from {31, 32, 33, 63, 64, 65, 130} in both orientations — the word rows of a packed bit box and the
encoder's 63-position chunks — and one 300x260 plane.  Contents: empty, full, a pixel in a corner, a mask on each border, a
checkerboard, a comb (full-height columns under a full top row: its runs wrap column ends), ellipses, a mask with pinholes and specks,
and inputs re-encoded with zero-length runs.  Radii 0, 1, 2, 31, 32, 33, 102 and one at least as large as a side."""
import importlib

import numpy as np

ERODE, DILATE, BOUNDARY = 0, 1, 2
OPS = {"erode": ERODE, "dilate": DILATE, "boundary": BOUNDARY}
RADII = [0, 1, 2, 31, 32, 33, 102]
SIDES = [31, 32, 33, 63, 64, 65, 130]
SHAPE, INVALID = 4, 1                        # MRCNN_ERR_SHAPE, MRCNN_ERR_INVALID


# ---- the rule on dense planes ------------------------------------------------------------------------------------------------------------
def _line(P, r, axis, grows):
    """one half of the square: the AND (erosion) or OR (dilation) of the 2r + 1 slices of the zero-padded plane along `axis`"""
    n = P.shape[axis]
    r = min(r, n)                            # a wider window sees nothing new: beyond the plane is all padding
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    Z = np.pad(P.astype(bool), pad)
    out = np.zeros(P.shape, bool) if grows else np.ones(P.shape, bool)
    for d in range(2 * r + 1):
        s = Z[d:d + n] if axis == 0 else Z[:, d:d + n]
        out = out | s if grows else out & s
    return out


def window_2d(P, r, grows):
    """the rule as it reads, the full (2r + 1)^2 window: for small r, to pin that the square is a column of 2r + 1 times a row of 2r + 1"""
    h, w = P.shape
    Z = np.pad(P.astype(bool), r)
    out = np.zeros(P.shape, bool) if grows else np.ones(P.shape, bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            s = Z[dy:dy + h, dx:dx + w]
            out = out | s if grows else out & s
    return out.astype(np.uint8)


def reference(P, r, op):
    """E_r(P), D_r(P) or P & ~E_r(P) as a uint8 plane; outside the image is 0"""
    grows = op == DILATE
    R = _line(_line(P, r, 0, grows), r, 1, grows)
    if op == BOUNDARY:
        R = P.astype(bool) & ~R
    return R.astype(np.uint8)


def reference_sat(P, r, op):
    """the same by a summed-area table: the window's count is (2r + 1)^2 (erosion) or positive (dilation).  O(h*w) whatever r: the cap case"""
    h, w = P.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(P.astype(np.int64), 0), 1)
    y0, y1 = np.clip(np.arange(h) - r, 0, h), np.clip(np.arange(h) + r + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) - r, 0, w), np.clip(np.arange(w) + r + 1, 0, w)
    count = S[y1][:, x1] - S[y0][:, x1] - S[y1][:, x0] + S[y0][:, x0]
    R = count > 0 if op == DILATE else count == (2 * r + 1) ** 2
    if op == BOUNDARY:
        R = P.astype(bool) & ~R
    return R.astype(np.uint8)


def published_boundary(P, d):
    """Boundary IoU's mask_to_boundary, restated literally: pad the mask by one ring of zeros, d iterations of a 3x3 erosion whose
    outside counts as set, un-pad, subtract from the mask"""
    h, w = P.shape
    M = np.pad(P.astype(bool), 1)
    for _ in range(d):
        Z = np.pad(M, 1, constant_values=True)
        E = np.ones(M.shape, bool)
        for dy in range(3):
            for dx in range(3):
                E &= Z[dy:dy + h + 2, dx:dx + w + 2]
        M = E
    return (P.astype(bool) & ~M[1:h + 1, 1:w + 1]).astype(np.uint8)


# ---- run lengths -------------------------------------------------------------------------------------------------------------------------
def encode(P):
    """the canonical column-major RLE of a plane: counts[0] the leading zeros (may be 0), no other run 0, [h*w] for an empty plane"""
    flat = np.asarray(P, np.uint8).T.reshape(-1)
    at = np.flatnonzero(np.diff(np.concatenate(([0], flat)))) if flat.size else np.zeros(0, np.int64)
    return np.diff(np.concatenate(([0], at, [flat.size]))).astype(np.uint32)


def decode(counts, h, w):
    flat = np.repeat(np.arange(len(counts)) & 1, np.asarray(counts, np.int64)).astype(np.uint8)
    assert flat.size == h * w
    return flat.reshape(w, h).T.copy()


def with_zero_runs(counts, rng, every=3):
    """the same plane with zero-length runs put in: two at the front, and every `every`-th run split around an empty run of the other kind"""
    out = [0, 0]
    for j, c in enumerate(np.asarray(counts, np.int64).tolist()):
        if j % every == 0:
            a = int(rng.integers(0, c + 1))
            out += [a, 0, c - a]
        else:
            out.append(c)
    return np.array(out, np.uint32)


def stats(P):
    """(area, [x, y, w, h]) as mrcnn_masks_rle_source states them"""
    ys, xs = np.nonzero(P)
    if ys.size == 0:
        return 0, [0, 0, 0, 0]
    return int(ys.size), [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


# ---- contents ----------------------------------------------------------------------------------------------------------------------------
def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - cy) / max(ry, 0.5)) ** 2 + ((xx - cx) / max(rx, 0.5)) ** 2) <= 1.0).astype(np.uint8)


def contents(h, w, rng):
    """[(name, plane)] for one size"""
    z = lambda: np.zeros((h, w), np.uint8)
    out = [("empty", z()), ("full", np.ones((h, w), np.uint8))]
    for name, (y, x) in (("corner_tl", (0, 0)), ("corner_tr", (0, w - 1)), ("corner_bl", (h - 1, 0)), ("corner_br", (h - 1, w - 1))):
        p = z(); p[y, x] = 1
        out.append((name, p))
    for name, (cy, cx) in (("top", (0, w / 2)), ("bottom", (h - 1, w / 2)), ("left", (h / 2, 0)), ("right", (h / 2, w - 1))):
        out.append((name, ellipse(h, w, cy, cx, h / 3, w / 3)))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", ((yy + xx) & 1).astype(np.uint8)))
    comb = z(); comb[:, ::2] = 1; comb[0, :] = 1
    out.append(("comb", comb))
    two = ellipse(h, w, h * 0.3, w * 0.3, h * 0.25, w * 0.2) | ellipse(h, w, h * 0.65, w * 0.7, h * 0.3, w * 0.25)
    out.append(("ellipses", two))
    holes = ellipse(h, w, h / 2, w / 2, h * 0.45, w * 0.45)
    holes &= ~(rng.random((h, w)) < 0.02).astype(np.uint8) & 1
    holes |= (rng.random((h, w)) < 0.01).astype(np.uint8)
    out.append(("pinholes_specks", holes))
    return out


SIZES = [(1, 1), (1, 7), (7, 1), (5, 5)] + [(a, b) for a, b in zip(SIDES, SIDES[3:] + SIDES[:3])] + [(b, a) for a, b in zip(SIDES, SIDES[3:] + SIDES[:3])] \
    + [(64, 64), (130, 130), (300, 260)]


def all_cases():
    """[(name, counts, h, w, r)]: every content of every size at two radii of RADII in turn and at one radius >= a side, the 300x260 plane at
    every radius, and every fourth input re-encoded with zero-length runs.  Deterministic."""
    rng = np.random.default_rng(11)
    out, turn = [], 0
    for h, w in SIZES:
        for name, plane in contents(h, w, rng):
            counts = encode(plane)
            radii = RADII + [300] if (h, w) == (300, 260) and name in ("ellipses", "pinholes_specks", "full", "comb") else \
                [RADII[turn % 7], RADII[(turn + 3) % 7]] + ([max(h, w) + (turn % 2)] if turn % 5 == 0 else [])
            for r in radii:
                c = with_zero_runs(counts, rng) if turn % 4 == 1 else counts
                out.append((f"{name}/{h}x{w}/r{r}" + ("/zero_runs" if c is not counts else ""), c, h, w, r))
                turn += 1
    return out


def flat_set(cases):
    """the cases as one ragged call: (counts, run_offsets, heights, widths, radii)"""
    counts = np.concatenate([c[1] for c in cases]).astype(np.uint32)
    offs = np.concatenate(([0], np.cumsum([len(c[1]) for c in cases]))).astype(np.int64)
    col = lambda i: np.array([c[i] for c in cases], np.int32)
    return counts, offs, col(2), col(3), col(4)


def cap_case():
    """2100x2100 with three set pixels, r = MRCNN_MORPH_MAX_RADIUS: the window is wider than any tile of the horizontal pass"""
    P = np.zeros((2100, 2100), np.uint8)
    P[0, 0] = P[1037, 1050] = P[2099, 30] = 1
    return P, 1024


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def morph_host(counts, offs, hs, ws, radii, op, capacity=None, fill=None):
    """mrcnn_rle_morph_host with the size query first -> (status, message, counts, run_offsets, areas, bboxes)"""
    lib = _lib()
    L = lib.lib()
    n = len(offs) - 1
    counts, offs = np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(offs, np.int64)
    hs, ws, radii = (np.ascontiguousarray(a, np.int32) for a in (hs, ws, radii))
    out_offs, areas, boxes = np.zeros(n + 1, np.int64), np.zeros(max(1, n), np.uint32), np.zeros((max(1, n), 4), np.int32)
    head = (counts.ctypes.data, offs.ctypes.data, n, hs.ctypes.data, ws.ctypes.data, radii.ctypes.data, op)
    if capacity is None:
        st = L.mrcnn_rle_morph_host(*head, None, 0, out_offs.ctypes.data, None, None)
        if st != SHAPE or out_offs[n] == 0:
            return st, L.mrcnn_last_error().decode(), None, out_offs, areas[:n], boxes[:n]
        capacity = int(out_offs[n])
    out = np.zeros(max(1, capacity), np.uint32) if fill is None else np.full(max(1, capacity), fill, np.uint32)
    st = L.mrcnn_rle_morph_host(*head, out.ctypes.data, capacity, out_offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data)
    return st, L.mrcnn_last_error().decode(), out[:int(out_offs[n])] if st == 0 else out, out_offs, areas[:n], boxes[:n]


def assert_same(got, want, what):
    """(counts, run_offsets, areas, bboxes) against the same four, numpy arrays or tensors"""
    host = lambda a: a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    for name, g, w_ in zip(("out_run_offsets", "out_counts", "areas", "bboxes_xywh"), (got[1], got[0], got[2], got[3]), (want[1], want[0], want[2], want[3])):
        g, w_ = host(g), host(w_)
        if name in ("out_counts", "areas"):
            g, w_ = g.view(np.uint32), w_.view(np.uint32)
        assert g.shape == w_.shape and (g == w_).all(), f"{what}: {name} differs" + (f" first at {int(np.flatnonzero((g != w_).reshape(-1))[0])}" if g.shape == w_.shape else f": shapes {g.shape} / {w_.shape}")
