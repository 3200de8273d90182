"""Shared by tests/test_polygons_simplify_host.py and tests/test_gpu_polygons_simplify.py: a restatement of the rule in
include/maskrcnn_hip.h (mrcnn_polygons_simplify), the rings both simplify, and the plumbing that calls the two entries on flat arrays.

The restatement shares nothing with csrc/simplify_host.cpp, csrc/simplify_rule.h or the kernels: it is recursive, works on Python
integers (no width to overflow, no 128-bit product to build), and takes E from math.floor(tol * tol * 65536)."""
import ctypes as C
import importlib
import math
import sys

import numpy as np

import polygons_cases as PC

INVALID, HIP, SHAPE = PC.INVALID, PC.HIP, PC.SHAPE
KEYS = ("ring_offsets", "areas2", "xy", "src_index")
TOLERANCES = (0, 0.25, 0.5, 1, 1.5, 3, 50, 65535)
E_MAX = 65535 * 65535 * 65536


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def tolerance_E(tol):
    return math.floor(tol * tol * 65536)


def distance(a, b, p):
    """the rule's distance of p from the chain ends a, b (tuples of Python ints)"""
    if a == b:
        return (p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2
    return abs((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]))


def within(a, b, c, E):
    """not farther than the tolerance: the negation of the rule's test for a vertex at distance c from the chord a .. b"""
    if a == b:
        return c * 65536 <= E
    return c * c * 65536 <= E * ((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2)


def restate_ring(ring, E, events=None):
    """the indices of the vertices of one ring ([(x, y)] of Python ints) that stay, increasing.  events: a set that receives what the
    ring met: "anchor_tie", "distance_tie" (a tie that was decided and kept), "a_equals_b", and the deepest level as ("depth", d)"""
    m = len(ring)
    if m <= 2:
        return list(range(m))
    events = set() if events is None else events
    v = list(ring) + [ring[0]]                                   # v[m] is v[0] again
    far = [(x - v[0][0]) ** 2 + (y - v[0][1]) ** 2 for x, y in ring]
    f = far.index(max(far))                                      # the smallest index of the largest
    if far.count(max(far)) > 1 and max(far) > 0:
        events.add("anchor_tie")
    kept = {0, f}

    def chain(i, j, depth=1):
        if j - i < 2:
            return
        events.add(("depth", depth))
        if v[i] == v[j]:
            events.add("a_equals_b")
        c = [distance(v[i], v[j], v[k]) for k in range(i + 1, j)]
        best = max(c)
        k = i + 1 + c.index(best)
        if within(v[i], v[j], best, E):
            return
        if c.count(best) > 1:
            events.add("distance_tie")
        kept.add(k)
        chain(i, k, depth + 1)
        chain(k, j, depth + 1)

    chain(0, f)
    chain(f, m)
    return sorted(kept)


def restate(ring_offsets, xy, tol):
    """the four arrays of the entry for flat rings, by the restatement"""
    E = tolerance_E(tol)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 100000))
    try:
        offs, areas2, out, src = [0], [], [], []
        for r in range(len(ring_offsets) - 1):
            v0 = int(ring_offsets[r])
            ring = [(int(x), int(y)) for x, y in xy[v0:int(ring_offsets[r + 1])]]
            idx = restate_ring(ring, E)
            pts = [ring[i] for i in idx]
            areas2.append(sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(pts, pts[1:] + pts[:1])))
            out.extend(pts)
            src.extend(v0 + i for i in idx)
            offs.append(len(out))
    finally:
        sys.setrecursionlimit(limit)
    return {"ring_offsets": np.array(offs, np.int64), "areas2": np.array(areas2, np.int64), "xy": np.array(out, np.int32).reshape(-1, 2),
            "src_index": np.array(src, np.int64)}


# ---- the rings ------------------------------------------------------------------------------------------------------------------
def flat_of(rings):
    """a list of (m, 2) integer arrays -> (ring_offsets, xy)"""
    rings = [np.asarray(r, np.int32).reshape(-1, 2) for r in rings]
    offs = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    return offs, (np.concatenate(rings) if rings else np.zeros((0, 2), np.int32)).astype(np.int32)


def disk(radius, cx=None, hole=0.0, ax=1.0, ay=1.0):
    """a staircase ellipse with half axes radius*ax, radius*ay (a disk by default), with a concentric hole of `hole` times its size"""
    c = int(radius * max(ax, ay)) + 2 if cx is None else cx
    yy, xx = np.indices((2 * c + 1, 2 * c + 1))
    d = ((xx - c) / ax) ** 2 + ((yy - c) / ay) ** 2
    return ((d <= radius * radius) & ((d > (hole * radius) ** 2) | (hole == 0))).astype(np.uint8)


def trace_planes(planes):
    """the host tracer's flat arrays for a list of planes"""
    return PC.trace_host([_cr().rle_encode(p) for p in planes])


# the four corners of the largest plane and vertices beside its diagonals: c reaches 32767^2, the most a cross product of such vertices can
# be, and c^2 * 65536 about 7.6e22, far beyond 64 bits; E * |b - a|^2 reaches 6e23 with the largest E
EXTREME = [(0, 0), (32767, 0), (32767, 32766), (32767, 32767), (16384, 16383), (0, 32767), (1, 16383), (16383, 16384)]
EXTREME_TOLERANCES = (0, 1, 23169, 23170, 32767, 65535)          # (32767, 0) lies 23169.8 from the diagonal: kept at 23169, dropped at 23170


def hand_made():
    """[(name, ring)]: integer rings that are not traced.

    A chain with a = b: under the ring rule it arises only when ALL vertices of a ring coincide.  A kept vertex has c > 0, so it differs
    from both ends of its chain, and v_f differs from v_0 unless every vertex equals v_0; by induction the two ends of every other
    chain differ.  "all_equal" rings are therefore the ones that reach the rule's second distance; a ring that passes twice through a
    vertex ("twice_through_a_vertex", "back_and_forth", and the traced rings with diagonal contacts) never does, whatever is kept."""
    return [
        ("m0", []), ("m1", [(5, 7)]), ("m2", [(1, 1), (4, 5)]), ("m3", [(0, 0), (4, 0), (0, 3)]), ("m4", [(0, 0), (4, 0), (4, 3), (0, 3)]),
        ("all_equal/3", [(3, 3), (3, 3), (3, 3)]), ("all_equal/6", [(9, 2)] * 6),
        ("rectangle", [(2, 1), (9, 1), (9, 6), (2, 6)]),
        ("twice_through_a_vertex", [(0, 0), (5, 5), (9, 2), (10, 0), (10, 10), (5, 5), (2, 9), (0, 10), (5, 5), (3, 4)]),
        ("back_and_forth", [(0, 0), (10, 0), (0, 0), (10, 0), (5, 1)]),
        # (6, 8), (10, 0), (8, 6) and (0, 10) are all 100 from the start: the first is the anchor
        ("anchor_tie", [(0, 0), (3, 1), (6, 8), (10, 0), (8, 6), (0, 10), (1, 3)]),
        # the anchors are (0, 4) and (8, 4); (2, 7) and (6, 7) are equally far from that chord, as are (6, 1) and (2, 1): the first of each pair is chosen
        ("distance_tie", [(0, 4), (2, 7), (4, 5), (6, 7), (8, 4), (6, 1), (4, 3), (2, 1)]),
        ("collinear", [(0, 0), (1, 0), (2, 0), (5, 0), (9, 0), (9, 4), (9, 9), (6, 6), (3, 3), (1, 1)]),
        ("collinear/all", [(0, 0), (3, 3), (5, 5), (9, 9), (7, 7), (2, 2)]),
        ("extreme", EXTREME),
    ]


_RINGS = []


def rings():
    """(names, ring_offsets, xy): every ring the CPU tests simplify, flat.  The rings polygons_cases.cases() traces, staircase disks and
    ellipses with and without holes, and the hand-made ones."""
    if _RINGS:
        return _RINGS[0]
    traced = PC.trace_host([r for _, r in PC.cases()])
    names = []
    for k, (name, _) in enumerate(PC.cases()):
        names += [f"{name}/ring{q}" for q in range(int(traced["rle_rings"][k + 1] - traced["rle_rings"][k]))]
    shapes = [("disk/12", disk(12)), ("disk/40.5", disk(40.5)), ("disk/40.5/hole", disk(40.5, hole=0.5)), ("ellipse", disk(30, ax=1.0, ay=0.4)),
              ("ellipse/hole", disk(25, ax=0.6, ay=1.3, hole=0.7))]
    t2 = trace_planes([p for _, p in shapes])
    for k, (name, _) in enumerate(shapes):
        names += [f"{name}/ring{q}" for q in range(int(t2["rle_rings"][k + 1] - t2["rle_rings"][k]))]
    hand = hand_made()
    names += [n for n, _ in hand]
    h_off, h_xy = flat_of([np.array(r, np.int32).reshape(-1, 2) for _, r in hand])
    V1, V2 = int(traced["n_vertices"]), int(t2["n_vertices"])
    offs = np.concatenate((traced["ring_offsets"], t2["ring_offsets"][1:] + V1, h_off[1:] + V1 + V2)).astype(np.int64)
    xy = np.concatenate((traced["xy"], t2["xy"], h_xy)).astype(np.int32)
    assert len(names) == len(offs) - 1
    _RINGS.append((names, offs, xy, int(traced["n_rings"])))
    return _RINGS[0]


# ---- the two entries on flat arrays ------------------------------------------------------------------------------------------------
def call_host(offs, xy, tol, capacity, fill=-7, null=False, n_rings=None, areas=True, src=True):
    """mrcnn_polygons_simplify_host on numpy arrays -> (status, message, arrays + the total)"""
    L = _lib().lib()
    R = len(offs) - 1 if n_rings is None else n_rings
    xy = np.ascontiguousarray(xy, np.int32)
    out = {"ring_offsets": np.full(max(1, R + 1), fill, np.int64), "areas2": np.full(max(1, R), fill, np.int64),
           "xy": np.full(max(1, 2 * capacity), fill, np.int32), "src_index": np.full(max(1, capacity), fill, np.int64)}
    total = C.c_int64(fill)
    p = lambda a, on=True: a.ctypes.data if on and not null else None
    xp = xy.ctypes.data if xy.size else np.zeros(2, np.int32).ctypes.data
    st = L.mrcnn_polygons_simplify_host(offs.ctypes.data, xp, R, C.c_double(tol), out["ring_offsets"].ctypes.data, p(out["areas2"], areas), p(out["xy"]),
                                        p(out["src_index"], src), C.byref(total), capacity)
    out["n_vertices"] = total.value
    return st, L.mrcnn_last_error().decode(), out


def cut(out, R):
    """the arrays of a call cut to their totals (xy as (V, 2))"""
    V = out["n_vertices"]
    return {"ring_offsets": out["ring_offsets"][:R + 1], "areas2": out["areas2"][:R], "xy": out["xy"][:2 * V].reshape(V, 2), "src_index": out["src_index"][:V],
            "n_vertices": V}


def simplify_host(offs, xy, tol):
    """The host definition: the size query, then the call.  -> arrays cut to their totals"""
    R = len(offs) - 1
    st, msg, q = call_host(offs, xy, tol, 0, null=True)
    assert st == (SHAPE if q["n_vertices"] else 0), msg
    st, msg, out = call_host(offs, xy, tol, q["n_vertices"])
    assert st == 0, msg
    assert out["n_vertices"] == q["n_vertices"] and np.array_equal(out["ring_offsets"], q["ring_offsets"])
    return cut(out, R)


def assert_same(got, want, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1), err_msg=f"{what} {key}")
