"""The cases of the shape-measure tests (tests/test_rle_shape_host.py, tests/test_gpu_rle_shape.py) and the rules of
include/maskrcnn_hip.h restated in numpy and Python ints on dense planes: the moments from np.nonzero, the perimeter from np.diff of the
zero-padded plane, the hull by a monotone chain over all four corners of every set pixel (on the few large planes the per-column
extremes stand in), the oriented box by the brute loop over edges and vertices with exact fractions.

Planes: 1x1, 1x9, 9x1, sides 31..33 against 63..65 in both orientations, and 1100x9.  Contents: empty, full, one corner pixel, four
corner pixels, two far pixels, a single column, a single row, a checkerboard, a comb (full-height columns under a full top row: its runs
wrap column ends), the diagonal and the anti-diagonal pixel staircases (many collinear candidates), an L, a cross, two ellipses, a mask
with empty columns in its middle, and random planes at densities 0.02, 0.5 and 0.9.  Every fourth RLE is re-encoded with zero-length
runs.  One call carries all planes of all sizes.  Deterministic."""
import ctypes as C
import importlib
from fractions import Fraction

import numpy as np

from morph_cases import decode, ellipse, encode, with_zero_runs  # noqa: F401  (decode is the tests')

SHAPE, INVALID = 4, 1                        # MRCNN_ERR_SHAPE, MRCNN_ERR_INVALID
SIZES = [(1, 1), (1, 9), (9, 1), (31, 63), (32, 64), (33, 65), (63, 31), (64, 32), (65, 33), (1100, 9)]
CONTENTS = ["empty", "full", "corner", "corners", "two_far", "column", "row", "checkerboard", "comb", "diagonal", "antidiagonal", "L", "cross",
            "ellipse_a", "ellipse_b", "gap", "rand002", "rand05", "rand09"]


# ---- the rules on dense planes -----------------------------------------------------------------------------------------------------------
def measures_of(P):
    """[S1, Sx, Sy, Sxx, Sxy, Syy, perimeter] of a plane, Python ints"""
    ys, xs = (a.astype(object) for a in np.nonzero(P))
    Z = np.pad(np.asarray(P, np.int64), 1)
    per = int(np.abs(np.diff(Z, axis=0)).sum() + np.abs(np.diff(Z, axis=1)).sum())
    s = lambda v: int(v.sum()) if len(v) else 0
    return [len(xs), s(xs), s(ys), s(xs * xs), s(xs * ys), s(ys * ys), per]


def chain_hull(points):
    """Andrew's monotone chain over integer points (x, y), strict: the ring with positive shoelace area — clockwise on a screen whose y
    points down — from the smallest point by x then y"""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return pts
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def hull_of(P, columns_only=False):
    """the hull of the set pixels' squares: all four corners of every set pixel, or (columns_only, for large planes) the corners of the
    first and the last set pixel of every column"""
    P = np.asarray(P)
    if columns_only:
        pts = []
        for x in np.flatnonzero(P.any(axis=0)):
            ys = np.flatnonzero(P[:, x])
            pts += [(x, ys[0]), (x + 1, ys[0]), (x, ys[-1] + 1), (x + 1, ys[-1] + 1)]
    else:
        ys, xs = np.nonzero(P)
        pts = [(x + dx, y + dy) for x, y in zip(xs.tolist(), ys.tolist()) for dx in (0, 1) for dy in (0, 1)]
    return chain_hull(pts)


def area2_of(ring):
    return sum(ring[i][0] * ring[(i + 1) % len(ring)][1] - ring[(i + 1) % len(ring)][0] * ring[i][1] for i in range(len(ring)))


def box_of(ring):
    """[e, dx, dy, dmin, dmax, cmin, cmax, 0] by the brute loop: the smallest D*C/L2 as an exact fraction, the smallest e on a tie"""
    if not ring:
        return [-1, 0, 0, 0, 0, 0, 0, 0]
    best = None
    for e in range(len(ring)):
        (ax, ay), (bx, by) = ring[e], ring[(e + 1) % len(ring)]
        dx, dy = bx - ax, by - ay
        d = [dx * x + dy * y for x, y in ring]
        c = [dx * y - dy * x for x, y in ring]
        area = Fraction((max(d) - min(d)) * (max(c) - min(c)), dx * dx + dy * dy)
        if best is None or area < best[0]:
            best = (area, [e, dx, dy, min(d), max(d), min(c), max(c), 0])
    return best[1]


def reference(planes, columns_only=False):
    """(measures (n, 7) as a list of int lists, hulls as lists of (x, y), areas2, obb rows) of a list of planes"""
    hulls = [hull_of(P, columns_only) for P in planes]
    return [measures_of(P) for P in planes], hulls, [area2_of(r) for r in hulls], [box_of(r) for r in hulls]


# ---- contents ----------------------------------------------------------------------------------------------------------------------------
def contents(h, w, rng):
    """the planes of one size, in CONTENTS' order"""
    z = lambda: np.zeros((h, w), np.uint8)
    corner = z(); corner[h - 1, 0] = 1
    corners = z(); corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 1
    far = z(); far[0, w - 1] = far[h - 1, 0] = 1
    column = z(); column[:, w // 2] = 1
    row = z(); row[h // 2, :] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    comb = z(); comb[:, ::2] = 1; comb[0, :] = 1
    diag, anti = z(), z()
    for i in range(min(h, w)):
        diag[i, i] = 1
        anti[i, w - 1 - i] = 1
    L = z(); L[:, 0:max(1, w // 5)] = 1; L[h - max(1, h // 5):, :] = 1
    cross = z(); cross[h // 3:h - h // 3, :] = 1; cross[:, w // 3:w - w // 3] = 1
    gap = z(); gap[h // 4:h // 2 + 1, 0:max(1, w // 4)] = 1; gap[h // 2:, w - max(1, w // 5):] = 1      # nothing between the two blocks
    out = [z(), np.ones((h, w), np.uint8), corner, corners, far, column, row, ((yy + xx) & 1).astype(np.uint8), comb, diag, anti, L, cross,
           ellipse(h, w, h * 0.45, w * 0.5, h * 0.35, w * 0.4), ellipse(h, w, h * 0.7, w * 0.3, h * 0.2, w * 0.25), gap]
    out += [(rng.random((h, w)) < d).astype(np.uint8) for d in (0.02, 0.5, 0.9)]
    return out


_CASES = None


def all_cases():
    """The whole set for one ragged call, made once: {"runs", "planes", "hs", "ws", "names": ["<content>/<h>x<w>"]}"""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(31)
        runs, planes, names = [], [], []
        for h, w in SIZES:
            for name, p in zip(CONTENTS, contents(h, w, rng)):
                c = encode(p)
                runs.append(with_zero_runs(c, rng) if len(runs) % 4 == 1 else c)
                planes.append(p)
                names.append(f"{name}/{h}x{w}")
        _CASES = {"runs": runs, "planes": planes, "names": names, "hs": np.array([p.shape[0] for p in planes], np.int32),
                  "ws": np.array([p.shape[1] for p in planes], np.int32)}
    return _CASES


_REFERENCE = None


def all_reference():
    """reference() of all_cases()' planes, computed once and shared"""
    global _REFERENCE
    if _REFERENCE is None:
        _REFERENCE = reference(all_cases()["planes"])
    return _REFERENCE


def flat_set(runs):
    """(counts, run_offsets) of a list of runs"""
    counts = np.concatenate(runs).astype(np.uint32) if len(runs) else np.zeros(1, np.uint32)
    return counts, np.concatenate(([0], np.cumsum([len(c) for c in runs]))).astype(np.int64)


def arch(h, w):
    """an arch over the whole width: a parabola's column tops down to the bottom row — a hull with many vertices on top, two below"""
    x = np.arange(w)
    top = np.rint((h - 1) * (2.0 * x / max(1, w - 1) - 1.0) ** 2).astype(np.int64)
    return (np.arange(h)[:, None] >= top[None, :]).astype(np.uint8)


def disc(side, radius):
    yy, xx = np.ogrid[0:side, 0:side]
    c = (side - 1) / 2.0
    return ((yy - c) ** 2 + (xx - c) ** 2 <= radius * radius).astype(np.uint8)


def full_measures(h, w):
    """the measures of the full h x w plane in closed form, Python ints"""
    s1 = lambda n: n * (n - 1) // 2
    s2 = lambda n: (n - 1) * n * (2 * n - 1) // 6
    return [h * w, s1(w) * h, s1(h) * w, s2(w) * h, s1(w) * s1(h), s2(h) * w, 2 * (h + w)]


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _head(counts, offs, hs, ws):
    counts, offs = np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(offs, np.int64)
    hs, ws = (np.ascontiguousarray(a, np.int32) for a in (hs, ws))
    return (counts, offs, hs, ws), (counts.ctypes.data, offs.ctypes.data, len(offs) - 1, hs.ctypes.data, ws.ctypes.data)


def measure_host(counts, offs, hs, ws, fill=0):
    """mrcnn_rle_measure_host -> (status, message, measures (n, 7))"""
    L = _lib().lib()
    keep, head = _head(counts, offs, hs, ws)
    n = len(offs) - 1
    out = np.full((max(1, n), 7), fill, np.int64)
    st = L.mrcnn_rle_measure_host(*head, out.ctypes.data)
    return st, L.mrcnn_last_error().decode(), out[:n]


def hull_host(counts, offs, hs, ws, capacity=None, fill=0):
    """mrcnn_rle_convex_hull_host, with the size query first unless a capacity is given -> (status, message, hull_offsets, xy (V, 2) — the
    whole pre-filled buffer when the call failed —, areas2, obb, n_vertices)"""
    L = _lib().lib()
    keep, head = _head(counts, offs, hs, ws)
    n = len(offs) - 1
    hull_offs, areas2, obb = np.full(n + 1, fill, np.int64), np.full(max(1, n), fill, np.int64), np.full((max(1, n), 8), fill, np.int64)
    nv = C.c_int64(fill)
    if capacity is None:
        st = L.mrcnn_rle_convex_hull_host(*head, hull_offs.ctypes.data, None, None, None, C.byref(nv), 0)
        if st != SHAPE or nv.value <= 0:
            return st, L.mrcnn_last_error().decode(), hull_offs, np.zeros((0, 2), np.int32), areas2[:n], obb[:n], int(nv.value)
        capacity = int(nv.value)
    xy = np.full((max(1, capacity), 2), fill, np.int32)
    st = L.mrcnn_rle_convex_hull_host(*head, hull_offs.ctypes.data, areas2.ctypes.data, obb.ctypes.data, xy.ctypes.data, C.byref(nv), capacity)
    return st, L.mrcnn_last_error().decode(), hull_offs, xy[:int(nv.value)] if st == 0 else xy, areas2[:n], obb[:n], int(nv.value)
