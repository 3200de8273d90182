"""Shared by tests/test_polygons_host.py and tests/test_gpu_polygons.py: the masks both trace, a naive restatement of the definition
in include/maskrcnn_hip.h (mrcnn_rle_to_polygons), and the plumbing that calls the two entries on flat arrays.

The restatement shares no method with csrc/polygons_host.cpp or the kernels: it lists the directed unit edges PIXEL BY PIXEL (the four
sides of every set pixel whose neighbour is unset) into a dictionary, follows them through that dictionary — right turn first, then
straight on, then left —, drops the collinear points and rotates every ring to its smallest vertex."""
import ctypes as C
import importlib

import numpy as np

INVALID, HIP, SHAPE = 1, 3, 4
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)                         # headings +x, +y, -x, -y: each the right turn of the one before


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def restate(plane):
    """(rings, areas) of one {0,1} plane: rings = [(m, 2) int32 arrays of x, y], ordered by start vertex; areas = int64."""
    p = np.asarray(plane) != 0
    h, w = p.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = p
    edges = {}                                                   # (x, y, heading) of every directed boundary edge -> walked?
    for y, x in zip(*np.nonzero(p)):
        x, y = int(x), int(y)
        if not pad[y, x + 1]:
            edges[(x, y, 0)] = False                             # top edge, +x
        if not pad[y + 1, x + 2]:
            edges[(x + 1, y, 1)] = False                         # right edge, +y
        if not pad[y + 2, x + 1]:
            edges[(x + 1, y + 1, 2)] = False                     # bottom edge, -x
        if not pad[y + 1, x]:
            edges[(x, y + 1, 3)] = False                         # left edge, -y
    rings = []
    for start in sorted(edges):
        if edges[start]:
            continue
        pts, e = [], start
        while not edges[e]:
            edges[e] = True
            x, y, d = e
            nx, ny = x + DX[d], y + DY[d]
            for turn in (1, 0, 3):                               # right, straight on, left
                nd = (d + turn) % 4
                if (nx, ny, nd) in edges:
                    break
            else:
                raise AssertionError("a boundary edge without a successor")
            if nd != d:
                pts.append((nx, ny))                             # a corner: the heading changes here
            e = (nx, ny, nd)
        assert e == start
        k = pts.index(min(pts))
        rings.append(np.array(pts[k:] + pts[:k], np.int32).reshape(-1, 2))
    rings.sort(key=lambda r: (int(r[0, 0]), int(r[0, 1])))
    areas = []
    for r in rings:
        x, y = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64)
        twice = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
        assert twice % 2 == 0
        areas.append(twice // 2)
    return rings, np.array(areas, np.int64)


def flat_arrays(per_rle):
    """[(rings, areas)] per RLE -> the four arrays of the C entry"""
    rle_rings, ring_offsets, areas, xy = [0], [0], [], []
    for rings, a in per_rle:
        for r in rings:
            xy.append(r)
            ring_offsets.append(ring_offsets[-1] + len(r))
        areas.extend(int(v) for v in a)
        rle_rings.append(len(areas))
    return {"rle_rings": np.array(rle_rings, np.int64), "ring_offsets": np.array(ring_offsets, np.int64), "ring_areas": np.array(areas, np.int64),
            "xy": np.concatenate(xy).astype(np.int32) if xy else np.zeros((0, 2), np.int32)}


# ---- the masks ------------------------------------------------------------------------------------------------------------------
def _plane_of_bits(bits, h, w):
    return np.array([(bits >> i) & 1 for i in range(h * w)], np.uint8).reshape(h, w)


def _nested():
    p = np.zeros((9, 11), np.uint8)
    p[1:8, 1:10] = 1
    p[2:7, 2:9] = 0
    p[3:6, 4:7] = 1
    p[4, 5] = 0
    return p


_CASES = []


def cases():
    """[(name, rle)]: every mask the CPU tests trace; rle = {"size": [h, w], "counts": uint32}"""
    if _CASES:
        return _CASES
    enc = _cr().rle_encode
    add = lambda name, plane: _CASES.append((name, enc(plane)))
    for bits in range(512):
        add(f"3x3/{bits}", _plane_of_bits(bits, 3, 3))
    for bits in range(16):
        add(f"2x2/{bits}", _plane_of_bits(bits, 2, 2))
    rng = np.random.default_rng(20)
    for i in range(300):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        density = (0.3, 0.5, 0.7, 0.9)[i % 4]
        add(f"random/{i}/{h}x{w}/{density}", rng.random((h, w)) < density)
    add("1x1/set", np.ones((1, 1))), add("1x1/unset", np.zeros((1, 1)))
    for n in (2, 7):
        line = (np.arange(n) % 3 != 1)
        add(f"1x{n}", line[None, :]), add(f"{n}x1", line[:, None])
    add("full", np.ones((6, 5))), add("empty", np.zeros((6, 5)))
    add("checkerboard", np.indices((8, 9)).sum(0) % 2), add("checkerboard/other", (np.indices((8, 9)).sum(0) + 1) % 2)
    add("hole_with_island", _nested())
    # not in normal form: zero-length runs anywhere, and runs of ones that cross a column end (a 4 x 5 plane)
    _CASES.append(("zero_length_runs", {"size": [4, 5], "counts": np.array([0, 0, 0, 3, 0, 0, 2, 0, 4, 0, 0, 2, 5, 0, 4, 0], np.uint32)}))
    _CASES.append(("crossing_column_ends", {"size": [4, 5], "counts": np.array([2, 11, 3, 4], np.uint32)}))
    return _CASES


# ---- the two entries on flat arrays ------------------------------------------------------------------------------------------------
def flatten(rles):
    """a list of RLEs -> (counts, run_offsets, heights, widths): one image per RLE, slots = 1"""
    counts = np.concatenate([np.asarray(r["counts"], np.uint32) for r in rles]) if rles else np.zeros(0, np.uint32)
    offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for r in rles]))).astype(np.int64)
    hs = np.array([r["size"][0] for r in rles], np.int32)
    ws = np.array([r["size"][1] for r in rles], np.int32)
    return counts, offs, hs, ws


def call_host(counts, offs, n_images, slots, hs, ws, ring_capacity, vertex_capacity, fill=None, null=False):
    """mrcnn_rle_to_polygons_host on numpy arrays with the given capacities -> (status, message, arrays + totals)"""
    L = _lib().lib()
    n = n_images * slots
    rle_rings = np.full(n + 1, -7, np.int64)
    ring_offsets = np.full(ring_capacity + 1, -7 if fill is None else fill, np.int64)
    ring_areas = np.full(max(1, ring_capacity), -7 if fill is None else fill, np.int64)
    xy = np.full(max(1, 2 * vertex_capacity), -7 if fill is None else fill, np.int32)
    n_rings, n_vertices = C.c_int64(-7), C.c_int64(-7)
    counts = np.ascontiguousarray(counts, np.uint32)
    cp = counts.ctypes.data if counts.size else np.zeros(1, np.uint32).ctypes.data
    st = L.mrcnn_rle_to_polygons_host(cp, offs.ctypes.data, n_images, slots, hs.ctypes.data, ws.ctypes.data, rle_rings.ctypes.data, C.byref(n_rings),
                                      C.byref(n_vertices), None if null else ring_offsets.ctypes.data, None if null else ring_areas.ctypes.data,
                                      ring_capacity, None if null else xy.ctypes.data, vertex_capacity)
    return st, L.mrcnn_last_error().decode(), {"rle_rings": rle_rings, "ring_offsets": ring_offsets, "ring_areas": ring_areas, "xy": xy,
                                               "n_rings": n_rings.value, "n_vertices": n_vertices.value}


def trace_host(rles, n_images=None, slots=1, hs=None, ws=None):
    """The host definition on a list of RLEs: the size query, then the call.  -> arrays cut to their totals (xy as (V, 2))"""
    if n_images is None:
        counts, offs, hs, ws = flatten(rles)
        n_images = len(rles)
    else:
        counts, offs, _, _ = flatten(rles)
    st, msg, q = call_host(counts, offs, n_images, slots, hs, ws, 0, 0, null=True)
    assert st == (SHAPE if q["n_vertices"] else 0), msg
    st, msg, out = call_host(counts, offs, n_images, slots, hs, ws, q["n_rings"], q["n_vertices"])
    assert st == 0, msg
    assert (out["n_rings"], out["n_vertices"]) == (q["n_rings"], q["n_vertices"]) and np.array_equal(out["rle_rings"], q["rle_rings"])
    R, V = out["n_rings"], out["n_vertices"]
    return {"rle_rings": out["rle_rings"], "ring_offsets": out["ring_offsets"][:R + 1], "ring_areas": out["ring_areas"][:R],
            "xy": out["xy"][:2 * V].reshape(V, 2), "n_rings": R, "n_vertices": V}


def rings_of(arrays, k):
    """the rings and areas of RLE k of flat arrays"""
    r0, r1 = int(arrays["rle_rings"][k]), int(arrays["rle_rings"][k + 1])
    ro = arrays["ring_offsets"]
    return [arrays["xy"][int(ro[r]):int(ro[r + 1])] for r in range(r0, r1)], arrays["ring_areas"][r0:r1]


def assert_same(got, want, what=""):
    for key in ("rle_rings", "ring_offsets", "ring_areas", "xy"):
        np.testing.assert_array_equal(np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1), err_msg=f"{what} {key}")
