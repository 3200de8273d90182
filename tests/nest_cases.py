"""Shared by tests/test_polygons_nest_host.py and tests/test_gpu_polygons_nest.py: the planes both nest, a restatement of the nesting
that shares no method with csrc/nest_rule.h, and the plumbing that calls the two entries of mrcnn_polygons_nest on flat arrays.

The restatement never looks at an edge.  It decodes the plane, pads it by one unset pixel and labels the set pixels 4-connected and
the unset pixels 8-connected (scipy.ndimage.label).  A ring's kind is the pixel (X0, Y0) at its start vertex — set: the outline of that
component, unset: the hole that component is — and must agree with the sign of the ring's area.  Its parent is read off the pixel
(X0 - 1, Y0) on the other side of the ring's first edge: for a hole the outline of that set component, for an outline the hole that
unset component is, or -1 when it is the outside.  The depth is a walk."""
import ctypes as C
import importlib

import numpy as np
from scipy import ndimage

import polygons_cases as PC

INVALID, HIP, SHAPE = 1, 3, 4


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def decode(rle):
    """the {0,1} plane of an RLE in any form: zero-length runs, runs that cross column ends"""
    h, w = int(rle["size"][0]), int(rle["size"][1])
    counts = np.asarray(rle["counts"], np.int64)
    bits = np.repeat(np.arange(len(counts)) % 2, counts).astype(np.uint8)
    assert bits.size == h * w
    return bits.reshape(w, h).T.copy()


def yardstick(plane, rings, areas):
    """(parent, depth) of the traced rings of one plane, local indices; see the module's docstring"""
    p = np.asarray(plane) != 0
    h, w = p.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = p
    set_lab, _ = ndimage.label(pad)                                                  # 4-connected
    unset_lab, _ = ndimage.label(~pad, structure=np.ones((3, 3), int))               # 8-connected
    outside = unset_lab[0, 0]
    outline_of, hole_of = {}, {}                                                     # component -> its ring
    for r, ring in enumerate(rings):
        x0, y0 = int(ring[0, 0]), int(ring[0, 1])
        if pad[y0 + 1, x0 + 1]:
            assert areas[r] > 0 and set_lab[y0 + 1, x0 + 1] not in outline_of
            outline_of[set_lab[y0 + 1, x0 + 1]] = r
        else:
            assert areas[r] < 0 and unset_lab[y0 + 1, x0 + 1] not in hole_of and unset_lab[y0 + 1, x0 + 1] != outside
            hole_of[unset_lab[y0 + 1, x0 + 1]] = r
    parent = np.full(len(rings), -1, np.int64)
    for r, ring in enumerate(rings):
        x0, y0 = int(ring[0, 0]), int(ring[0, 1])                                    # the pixel left of the first edge: padded index (y0 + 1, x0)
        if areas[r] < 0:
            assert pad[y0 + 1, x0]
            parent[r] = outline_of[set_lab[y0 + 1, x0]]
        else:
            assert not pad[y0 + 1, x0]
            lab = unset_lab[y0 + 1, x0]
            parent[r] = -1 if lab == outside else hole_of[lab]
    depth = np.zeros(len(rings), np.int32)
    for r in range(len(rings)):
        q, steps = parent[r], 0
        while q >= 0:
            q, steps = parent[q], steps + 1
            assert steps <= len(rings)
        depth[r] = steps
    return parent, depth


def grouping(parent, depth, rle_rings):
    """rle_polys, poly_rings, ring_order from parent and depth (global indices), as the header words them"""
    parent, depth = np.asarray(parent), np.asarray(depth)
    rle_polys, poly_rings, order = [0], [], []
    for k in range(len(rle_rings) - 1):
        for r in range(int(rle_rings[k]), int(rle_rings[k + 1])):
            if depth[r] % 2:
                continue
            poly_rings.append(len(order))
            order.append(r)
            order.extend(int(q) for q in np.nonzero(parent == r)[0])
        rle_polys.append(len(poly_rings))
    poly_rings.append(len(order))
    return {"rle_polys": np.array(rle_polys, np.int64), "poly_rings": np.array(poly_rings, np.int64), "ring_order": np.array(order, np.int64),
            "n_polys": len(poly_rings) - 1}


def restate(traced, planes):
    """the nesting of traced flat arrays (one plane per RLE) by the yardstick"""
    rr = traced["rle_rings"]
    parent, depth = np.full(traced["n_rings"], -1, np.int64), np.zeros(traced["n_rings"], np.int32)
    for k, plane in enumerate(planes):
        rings, areas = PC.rings_of(traced, k)
        p, d = yardstick(plane, rings, areas)
        r0 = int(rr[k])
        parent[r0:r0 + len(p)] = np.where(p >= 0, p + r0, -1)
        depth[r0:r0 + len(p)] = d
    return {"parent": parent, "depth": depth, **grouping(parent, depth, rr)}


# ---- the planes ------------------------------------------------------------------------------------------------------------------
def _concentric():
    p = np.zeros((23, 23), np.uint8)
    for d in range(12):                                          # squares one pixel apart: rings of depth 0 .. 11
        p[d:23 - d, d:23 - d] = (d + 1) % 2
    return p


def _two_shells():
    p = np.zeros((12, 24), np.uint8)
    p[1:11, 1:11] = 1
    p[2:5, 2:5] = 0
    p[6:10, 3:9] = 0
    p[7:9, 5:7] = 1                                              # an island in the second hole
    p[1:11, 13:23] = 1
    p[2:4, 14:16] = 0
    p[5:9, 17:21] = 0
    return p


def _island_diagonal_to_its_hole():
    p = np.ones((7, 7), np.uint8)
    p[2:5, 2:5] = 0
    p[2, 2] = 1                                                  # the outline reaches into the hole's corner...
    p[3, 3] = 1                                                  # ...and the island touches it there, at the vertex (3, 3), and nowhere else
    return p


def _hole_diagonal_to_the_outside():
    p = np.ones((7, 7), np.uint8)
    p[0, 0] = 0                                                  # a corner cut out of the plane...
    p[1:3, 1:3] = 0                                              # ...and unset pixels that touch it only at the vertex (1, 1): 8-connected, so the outside
    return p


def _c_shape():
    p = np.zeros((11, 12), np.uint8)
    p[1:10, 1:10] = 1
    p[3:7, 3:10] = 0                                             # the mouth opens to the right
    p[4:6, 5:8] = 1                                              # a blob in the mouth: its probe lies inside the C's bounding box and outside the C
    return p


def _comb(teeth=520):
    """a comb whose outline has more than 2048 vertices, with a one-pixel hole in every tooth"""
    p = np.zeros((8, 4 * teeth + 1), np.uint8)
    p[5:7, :] = 1                                                # the back
    for t in range(teeth):
        p[0:5, 4 * t:4 * t + 3] = 1
        p[2, 4 * t + 1] = 0
    return p


_EXTRA = []


def extra_cases():
    """[(name, rle)]: the planes the issue of the nesting adds to polygons_cases.cases()"""
    if _EXTRA:
        return _EXTRA
    enc = _cr().rle_encode
    add = lambda name, plane: _EXTRA.append((name, enc(np.asarray(plane, np.uint8))))
    add("concentric", _concentric())
    add("two_shells", _two_shells())
    add("island_diagonal_to_its_hole", _island_diagonal_to_its_hole()), add("hole_diagonal_to_the_outside", _hole_diagonal_to_the_outside())
    add("c_shape", _c_shape())
    add("checkerboard/40x41", np.indices((40, 41)).sum(0) % 2)
    add("comb", _comb())
    return _EXTRA


def all_cases():
    return list(PC.cases()) + list(extra_cases())


SMALL = ("concentric", "two_shells", "island_diagonal_to_its_hole", "hole_diagonal_to_the_outside", "c_shape", "hole_with_island",
         "checkerboard", "checkerboard/other", "full", "zero_length_runs", "crossing_column_ends")


def ragged_set():
    """3 images x 4 slots with empty slots in the middle and at both ends -> (rles as rows, sizes, planes in RLE order)"""
    enc = _cr().rle_encode
    c = dict(all_cases())
    sizes = [(12, 24), (7, 7), (23, 23)]
    empty = lambda b: enc(np.zeros(sizes[b], np.uint8))
    rows = [[empty(0), c["two_shells"], empty(0), c["two_shells"]],
            [c["island_diagonal_to_its_hole"], empty(1), empty(1), c["hole_diagonal_to_the_outside"]],
            [c["concentric"], empty(2), c["concentric"], empty(2)]]
    return rows, sizes, [decode(r) for row in rows for r in row]


# ---- the two entries on flat arrays ------------------------------------------------------------------------------------------------
KEYS = ("parent", "depth", "rle_polys", "poly_rings", "ring_order")


def call(entry, rle_rings, ring_offsets, xy, fill=-9, memspace=None, n_rles=None, n_rings=None, null=()):
    """mrcnn_polygons_nest(_host) on numpy arrays -> (status, message, the five arrays sentinel-filled behind what was written, n_polys)"""
    lib = _lib()
    L = lib.lib()
    K = len(rle_rings) - 1 if n_rles is None else n_rles
    R = len(ring_offsets) - 1 if n_rings is None else n_rings
    size = max(1, len(ring_offsets) - 1)
    out = {"parent": np.full(size, fill, np.int64), "depth": np.full(size, fill, np.int32), "rle_polys": np.full(len(rle_rings), fill, np.int64),
           "poly_rings": np.full(size + 1, fill, np.int64), "ring_order": np.full(size, fill, np.int64)}
    total = C.c_int64(fill)
    xy = np.ascontiguousarray(xy, np.int32)
    args = {"rle_rings": np.ascontiguousarray(rle_rings, np.int64), "ring_offsets": np.ascontiguousarray(ring_offsets, np.int64),
            "xy": xy if xy.size else np.zeros(2, np.int32)}
    p = lambda name, a: None if name in null else a.ctypes.data
    mem = () if entry.endswith("_host") else (lib.HOST if memspace is None else memspace,)
    st = getattr(L, entry)(p("rle_rings", args["rle_rings"]), K, p("ring_offsets", args["ring_offsets"]), p("xy", args["xy"]), R, *mem,
                           *(p(k, out[k]) for k in KEYS), None if "n_polys" in null else C.byref(total))
    out["n_polys"] = total.value
    return st, L.mrcnn_last_error().decode(), out


def nest_host(arrays):
    """The host definition on traced (or any) flat arrays -> the five arrays cut to their sizes, and n_polys"""
    st, msg, out = call("mrcnn_polygons_nest_host", arrays["rle_rings"], arrays["ring_offsets"], arrays["xy"])
    assert st == 0, msg
    return cut(out, len(arrays["ring_offsets"]) - 1)


def cut(out, R):
    P = out["n_polys"]
    return {"parent": out["parent"][:R], "depth": out["depth"][:R], "rle_polys": out["rle_polys"], "poly_rings": out["poly_rings"][:P + 1],
            "ring_order": out["ring_order"][:R], "n_polys": P}


def assert_same(got, want, what=""):
    host = lambda a: a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    for key in KEYS:
        np.testing.assert_array_equal(host(got[key]).reshape(-1), host(want[key]).reshape(-1), err_msg=f"{what} {key}")
    assert int(got["n_polys"]) == int(want["n_polys"]), what


def assert_invariants(N, arrays, traced=True):
    """what the header states of every nesting; for traced rings also even depth <=> area > 0"""
    R = len(arrays["ring_offsets"]) - 1
    parent, depth, order, pr, rp, rr = N["parent"], N["depth"], N["ring_order"], N["poly_rings"], N["rle_polys"], arrays["rle_rings"]
    assert sorted(order.tolist()) == list(range(R))
    has = parent >= 0
    assert (depth[has] == depth[parent[has]] + 1).all() and (depth[~has] == 0).all()
    owner = np.searchsorted(rr, np.arange(R), side="right") - 1
    assert (owner[parent[has]] == owner[has]).all()                                  # never across RLEs
    assert rp[0] == 0 and rp[-1] == N["n_polys"] == len(pr) - 1 and pr[0] == 0 and pr[-1] == R and (np.diff(rp) >= 0).all()
    shells = []
    for p in range(N["n_polys"]):
        mine = order[pr[p]:pr[p + 1]]
        shell, holes = int(mine[0]), mine[1:]
        assert depth[shell] % 2 == 0
        np.testing.assert_array_equal(holes, np.nonzero(parent == shell)[0])           # exactly its children, in index order
        shells.append(shell)
    assert shells == sorted(shells) == np.nonzero(depth % 2 == 0)[0].tolist()
    for k in range(len(rr) - 1):
        assert all(rr[k] <= s < rr[k + 1] for s in shells[rp[k]:rp[k + 1]])
    if traced:
        assert ((depth % 2 == 0) == (arrays["ring_areas"] > 0)).all()
