"""The cases of the connected-component tests (tests/test_rle_components_host.py, tests/test_gpu_rle_components.py) and a numpy
restatement of the rule of include/maskrcnn_hip.h on dense planes: a union-find over the PIXELS of the labelled value — hook the
larger root of every neighbouring pair under the smaller, compress, repeat — whose roots are the components' first pixels in
column-major order.  Nothing but numpy.

Planes: 1x1, 1x7 and 7x1 (with h = 1 a run over five columns is five pieces that must unite), 5x5, two pixels that touch only
diagonally (the 4 / 8 difference, and the dual for zeros), a diagonal line, U and inverted U (they merge late), a one-pixel spiral
33x33 (a long chain), two interleaved spirals, nested rings (ring, hole, island, hole in the island), a checkerboard 64x64, a comb
whose runs wrap column ends, a piece ending at the bottom of column x beside one starting at the top of column x + 1 (different
components whose runs MERGE must join), empty and full planes, every content of tests/morph_cases.py at sides from {31, 32, 33, 63,
64, 65, 130} in both orientations, random planes 300x260 at densities 0.3, 0.5 and 0.6, planes of PIECES_THRESHOLD - 1,
PIECES_THRESHOLD and PIECES_THRESHOLD + 1 column pieces, and two inputs of every three re-encoded with zero-length runs."""
import importlib

import numpy as np

import morph_cases as MC

ONES, ZEROS = 1, 0
MERGE, SPLIT = 0, 1
SHAPE, INVALID, HIP = 4, 1, 3                # MRCNN_ERR_SHAPE, MRCNN_ERR_INVALID, MRCNN_ERR_HIP
PIECES_THRESHOLD = 1024                      # the piece count at which a workgroup-local labelling would have to hand over to the global one
COMBOS = [(ONES, 4), (ONES, 8), (ZEROS, 4), (ZEROS, 8)]


# ---- the rule on dense planes ------------------------------------------------------------------------------------------------------------
def label(P, connectivity, of):
    """(labels, n): labels[y, x] = the number of the component of pixel (y, x), -1 for a pixel of the other value; components of
    ones use `connectivity`, components of zeros the dual; numbered by their first pixel in column-major position x*h + y"""
    h, w = P.shape
    conn = connectivity if of == ONES else 12 - connectivity
    F = (np.asarray(P).T == of)                                  # (w, h): flat index = the column-major position
    idx = np.arange(h * w, dtype=np.int64).reshape(w, h)
    pairs = [(F[:, :-1] & F[:, 1:], idx[:, :-1], idx[:, 1:]), (F[:-1] & F[1:], idx[:-1], idx[1:])]
    if conn == 8:
        pairs += [(F[:-1, :-1] & F[1:, 1:], idx[:-1, :-1], idx[1:, 1:]), (F[:-1, 1:] & F[1:, :-1], idx[:-1, 1:], idx[1:, :-1])]
    a = np.concatenate([i[m] for m, i, _ in pairs])
    b = np.concatenate([j[m] for m, _, j in pairs])
    parent = np.arange(h * w, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        m = lo != hi
        if not m.any():
            break
        np.minimum.at(parent, hi[m], lo[m])                      # hook the larger root under the smaller
        while True:                                              # compress: every pixel points at its root
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    flat = F.reshape(-1)
    roots = np.flatnonzero(flat & (parent == np.arange(h * w)))  # rising position: the rule's order
    number = np.full(h * w, -1, np.int64)
    number[roots] = np.arange(len(roots))
    labels = np.where(flat, number[parent], -1)
    return labels.reshape(w, h).T.copy(), len(roots)


def measures(P, connectivity, of):
    """(areas, bboxes (C, 4) x y w h, flags) of the components of one plane"""
    h, w = P.shape
    L, n = label(P, connectivity, of)
    areas, boxes, flags = np.zeros(n, np.uint32), np.zeros((n, 4), np.int32), np.zeros(n, np.uint8)
    ys, xs = np.nonzero(L >= 0)
    c = L[ys, xs]
    areas[:] = np.bincount(c, minlength=n)
    for k, (lo, hi) in enumerate(((xs, xs), (ys, ys))):
        mn, mx = np.full(n, 1 << 30), np.full(n, -1)
        np.minimum.at(mn, c, lo), np.maximum.at(mx, c, hi)
        boxes[:, k], boxes[:, k + 2] = mn, mx - mn + 1
    x2, y2 = boxes[:, 0] + boxes[:, 2] - 1, boxes[:, 1] + boxes[:, 3] - 1
    flags[:] = (boxes[:, 0] == 0) | (boxes[:, 1] == 0) | (x2 == w - 1) | (y2 == h - 1)
    return areas, boxes, flags


def merged(P, connectivity, of, keep):
    """MERGE: the pixels of a dropped component take the other value"""
    L, n = label(P, connectivity, of)
    assert len(keep) == n
    R = np.array(P, np.uint8)
    if n == 0:
        return R
    drop = (L >= 0) & ~np.asarray(keep, bool)[np.maximum(L, 0)]
    R[drop] = 1 - of
    return R


def split(P, connectivity, keep):
    """SPLIT: one plane per kept component of ones, in component order"""
    L, n = label(P, connectivity, ONES)
    assert len(keep) == n
    return [(L == c).astype(np.uint8) for c in range(n) if keep[c]]


def split_counts(P, connectivity, keep):
    """SPLIT as canonical run lengths, one per kept component of ones, without a plane per component: the component's positions,
    cut where they stop being neighbours"""
    h, w = P.shape
    L, n = label(P, connectivity, ONES)
    assert len(keep) == n
    flat = L.T.reshape(-1)
    pos = np.flatnonzero(flat >= 0)
    order = np.argsort(flat[pos], kind="stable")
    pos, first = pos[order], np.searchsorted(flat[pos][order], np.arange(n + 1))
    out = []
    for c in range(n):
        if not keep[c]:
            continue
        p = pos[first[c]:first[c + 1]]
        cut = np.flatnonzero(np.diff(p) != 1)
        bounds = np.stack((p[np.concatenate(([0], cut + 1))], p[np.concatenate((cut, [len(p) - 1]))] + 1), 1).reshape(-1)
        runs = np.diff(np.concatenate(([0], bounds, [h * w])))
        out.append((runs[:-1] if bounds[-1] == h * w else runs).astype(np.uint32))
    return out


# ---- contents ----------------------------------------------------------------------------------------------------------------------------
def spiral(n, pitch=2):
    """(plane, area): a one-pixel line that winds inwards from (0, 0), `pitch` pixels between its arms; the area is the sum of the
    segments as they are drawn"""
    P = np.zeros((n, n), np.uint8)
    t, l, b, r = 0, 0, n - 1, n - 1
    x0, area = 0, 0
    while x0 <= r:
        P[t, x0:r + 1] = 1; area += r + 1 - x0                   # right along the top
        if t + 1 > b:
            break
        P[t + 1:b + 1, r] = 1; area += b - t                     # down the right side
        if l > r - 1:
            break
        P[b, l:r] = 1; area += r - l                             # left along the bottom
        if t + pitch > b - 1:
            break
        P[t + pitch:b, l] = 1; area += b - t - pitch             # up the left side, to `pitch` below the top arm
        x0 = l + 1
        t, l, b, r = t + pitch, l + pitch, b - pitch, r - pitch
    return P, area


def two_spirals(n):
    """two spirals of pitch 4, the second between the arms of the first"""
    P = spiral(n, 4)[0]
    P[2:n - 2, 2:n - 2] |= spiral(n - 4, 4)[0]
    return P


def rings(n):
    """square outlines at offsets 0, 3, 6, ..: ring, hole, island, hole in the island, .."""
    P = np.zeros((n, n), np.uint8)
    for o in range(0, n // 2, 3):
        P[o, o:n - o] = P[n - 1 - o, o:n - o] = 1
        P[o:n - o, o] = P[o:n - o, n - 1 - o] = 1
    return P


def pieces_plane(count):
    """single pixels on every second row of 64-row columns: `count` column pieces of ones, none touching (4) another"""
    w = (count + 31) // 32
    P = np.zeros((64, 2 * w), np.uint8)
    for i in range(count):
        P[2 * (i % 32), 2 * (i // 32)] = 1
    return P


def specials():
    z = lambda h, w: np.zeros((h, w), np.uint8)
    out = [("one_by_one_set", np.ones((1, 1), np.uint8)), ("one_by_one_clear", z(1, 1))]
    p = z(1, 7); p[0, 1:6] = 1
    out.append(("row_run_over_five_columns", p))
    p = z(7, 1); p[1:3, 0] = 1; p[5:, 0] = 1
    out.append(("column_two_pieces", p))
    p = z(5, 5); p[1:4, 1:4] = 1; p[2, 2] = 0
    out.append(("five_ring", p))
    p = z(5, 5); p[1, 1] = p[2, 2] = 1
    out.append(("diagonal_pair", p))
    p = z(5, 5); p[2, 1] = p[1, 2] = 1
    out.append(("antidiagonal_pair", p))
    out.append(("diagonal_line", np.eye(17, dtype=np.uint8)))
    out.append(("antidiagonal_line", np.eye(17, dtype=np.uint8)[::-1].copy()))
    p = z(12, 9); p[:, 1] = p[:, 7] = 1; p[11, 1:8] = 1
    out.append(("u", p))
    out.append(("inverted_u", p[::-1].copy()))
    out.append(("spiral_33", spiral(33)[0]))
    out.append(("spiral_34", spiral(34)[0]))
    out.append(("two_spirals_41", two_spirals(41)))
    out.append(("rings_21", rings(21)))
    out.append(("rings_40", rings(40)))
    yy, xx = np.mgrid[0:64, 0:64]
    out.append(("checkerboard_64", ((yy + xx) & 1).astype(np.uint8)))
    out.append(("checkerboard_64_inverse", ((yy + xx + 1) & 1).astype(np.uint8)))
    p = z(6, 5); p[4:, 1] = 1; p[:2, 2] = 1
    out.append(("bottom_beside_top", p))
    p = z(2, 3); p[1, 0] = 1; p[0, 1] = 1
    out.append(("bottom_beside_top_two_rows", p))
    p = z(1, 9); p[0, ::2] = 1
    out.append(("row_alternating", p))
    p = np.ones((6, 5), np.uint8); p[5, 1] = 0; p[0, 2] = 0
    out.append(("zeros_bottom_beside_top", p))
    rng = np.random.default_rng(5)
    for d in (0.3, 0.5, 0.6):
        out.append((f"random_{d}", (rng.random((300, 260)) < d).astype(np.uint8)))
    for c in (PIECES_THRESHOLD - 1, PIECES_THRESHOLD, PIECES_THRESHOLD + 1):
        out.append((f"pieces_{c}", pieces_plane(c)))
        out.append((f"pieces_{c}_inverse", 1 - pieces_plane(c)))
    return out


def all_cases():
    """[(name, counts, h, w, plane)]: the specials, every content of morph_cases at every size of morph_cases, and two inputs of
    every three once more with zero-length runs.  Deterministic."""
    rng = np.random.default_rng(23)
    planes = specials()
    for h, w in MC.SIZES:
        planes += [(f"{name}/{h}x{w}", p) for name, p in MC.contents(h, w, rng)]
    out = []
    for i, (name, p) in enumerate(planes):
        c = MC.encode(p)
        out.append((name, c, p.shape[0], p.shape[1], p))
        if i % 3 != 2:
            out.append((name + "/zero_runs", MC.with_zero_runs(c, rng), p.shape[0], p.shape[1], p))
    return out


def flat_set(cases):
    """the cases as one ragged call: (counts, run_offsets, heights, widths)"""
    counts = np.concatenate([c[1] for c in cases]).astype(np.uint32)
    offs = np.concatenate(([0], np.cumsum([len(c[1]) for c in cases]))).astype(np.int64)
    return counts, offs, np.array([c[2] for c in cases], np.int32), np.array([c[3] for c in cases], np.int32)


def large_case():
    """2100x2100: a one-pixel spiral in the upper left 1400x1400 and a field of specks beside and below it -> (plane, the spiral's area)"""
    P = np.zeros((2100, 2100), np.uint8)
    S, area = spiral(1400)
    P[:1400, :1400] = S
    rng = np.random.default_rng(9)
    specks = (rng.random((2100, 2100)) < 0.02).astype(np.uint8)
    specks[:1402, :1402] = 0
    return P | specks, area


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _set(counts, offs, hs, ws):
    counts, offs = np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(offs, np.int64)
    hs, ws = np.ascontiguousarray(hs, np.int32), np.ascontiguousarray(ws, np.int32)
    return (counts, offs, hs, ws), (counts.ctypes.data, offs.ctypes.data, len(offs) - 1, hs.ctypes.data, ws.ctypes.data)


def components_host(counts, offs, hs, ws, connectivity, of, capacity=None, fill=0):
    """mrcnn_rle_components_host with the size query first -> (status, message, comp_offsets, areas, bboxes, flags)"""
    L = _lib().lib()
    alive, head = _set(counts, offs, hs, ws)
    n = len(offs) - 1
    comp_offs = np.full(n + 1, fill, np.int64)
    if capacity is None:
        st = L.mrcnn_rle_components_host(*head, connectivity, of, comp_offs.ctypes.data, None, None, None, 0)
        if st not in (0, SHAPE) or (st == SHAPE and comp_offs[n] == fill):
            return st, L.mrcnn_last_error().decode(), comp_offs, None, None, None
        capacity = int(comp_offs[n])
    areas, boxes, flags = np.full(max(1, capacity), fill, np.uint32), np.full((max(1, capacity), 4), fill, np.int32), np.full(max(1, capacity), fill, np.uint8)
    st = L.mrcnn_rle_components_host(*head, connectivity, of, comp_offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data, flags.ctypes.data, capacity)
    C_ = int(comp_offs[n]) if st == 0 else capacity
    return st, L.mrcnn_last_error().decode(), comp_offs, areas[:C_], boxes[:C_], flags[:C_]


def select_host(counts, offs, hs, ws, connectivity, of, keep, mode, capacity=None):
    """mrcnn_rle_components_select_host with the size query first -> (status, message, counts, run_offsets, areas, bboxes, parent)"""
    import ctypes as C
    L = _lib().lib()
    alive, head = _set(counts, offs, hs, ws)
    n = len(offs) - 1
    keep = np.ascontiguousarray(keep, np.uint8)
    room = len(keep) if mode == SPLIT else n
    out_offs, areas, boxes, parent = np.zeros(room + 1, np.int64), np.zeros(max(1, room), np.uint32), np.zeros((max(1, room), 4), np.int32), np.zeros(max(1, room), np.int64)
    out_n = C.c_int64(-1)
    sel = (connectivity, of, keep.ctypes.data if len(keep) else None, len(keep), mode)
    if capacity is None:
        st = L.mrcnn_rle_components_select_host(*head, *sel, None, 0, out_offs.ctypes.data, None, None, parent.ctypes.data, C.byref(out_n))
        if st != SHAPE or out_n.value < 0:
            return st, L.mrcnn_last_error().decode(), None, out_offs, areas, boxes, parent
        capacity = int(out_offs[out_n.value])
    out = np.zeros(max(1, capacity), np.uint32)
    st = L.mrcnn_rle_components_select_host(*head, *sel, out.ctypes.data, capacity, out_offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data,
                                            parent.ctypes.data, C.byref(out_n))
    m = max(0, int(out_n.value))
    return st, L.mrcnn_last_error().decode(), out[:int(out_offs[m])] if st == 0 else out, out_offs[:m + 1], areas[:m], boxes[:m], parent[:m]


def assert_same(got, want, names, what):
    """arrays against arrays, numpy or tensors, bit for bit"""
    host = lambda a: a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    for name, g, w_ in zip(names, got, want):
        g, w_ = host(g), host(w_)
        if g.dtype.itemsize == 4 and w_.dtype.itemsize == 4:
            g, w_ = g.view(np.uint32), w_.view(np.uint32)
        assert g.shape == w_.shape and (g == w_).all(), f"{what}: {name} differs" + \
            (f" first at {int(np.flatnonzero((g != w_).reshape(-1))[0])}" if g.shape == w_.shape else f": shapes {g.shape} / {w_.shape}")


# ---- argument errors: (entry, changed arguments, status, a word of the message) -----------------------------------------------------------
MEASURE_ARGS = ("counts", "run_offsets", "n", "heights", "widths", "connectivity", "of", "memspace", "comp_offsets", "comp_areas", "comp_bboxes_xywh", "comp_flags",
                "comp_capacity")
SELECT_ARGS = ("counts", "run_offsets", "n", "heights", "widths", "connectivity", "of", "keep", "n_comps", "mode", "memspace", "out_counts", "capacity",
               "out_run_offsets", "areas", "bboxes_xywh", "out_parent", "out_n")
ARGUMENT_ERRORS = [
    ("measure", {"n": -1}, SHAPE, "n -1 is negative"),
    ("measure", {"run_offsets": None}, INVALID, "null argument"),
    ("measure", {"heights": None}, INVALID, "null argument"),
    ("measure", {"widths": None}, INVALID, "null argument"),
    ("measure", {"comp_offsets": None}, INVALID, "null comp_offsets"),
    ("measure", {"comp_areas": None}, INVALID, "null component array"),
    ("measure", {"comp_flags": None}, INVALID, "null component array"),
    ("measure", {"comp_capacity": -1}, INVALID, "comp_capacity -1"),
    ("measure", {"connectivity": 6}, SHAPE, "connectivity 6"),
    ("measure", {"of": -1}, SHAPE, "unknown of -1"),
    ("measure", {"memspace": 7}, INVALID, "unknown memspace 7"),
    ("select", {"n": -1}, SHAPE, "n -1 is negative"),
    ("select", {"n_comps": -1}, SHAPE, "n_comps -1 is negative"),
    ("select", {"run_offsets": None}, INVALID, "null argument"),
    ("select", {"heights": None}, INVALID, "null argument"),
    ("select", {"keep": None}, INVALID, "null argument"),
    ("select", {"out_n": None}, INVALID, "null argument"),
    ("select", {"out_run_offsets": None}, INVALID, "null argument"),
    ("select", {"out_parent": None, "mode": SPLIT}, INVALID, "null argument"),
    ("select", {"out_counts": None}, INVALID, "null out_counts with capacity"),
    ("select", {"capacity": -1}, INVALID, "capacity -1"),
    ("select", {"mode": 2}, SHAPE, "unknown mode 2"),
    ("select", {"of": ZEROS, "mode": SPLIT}, SHAPE, "SPLIT"),
    ("select", {"connectivity": 0}, SHAPE, "connectivity 0"),
    ("select", {"memspace": 7}, INVALID, "unknown memspace 7"),
]


def call_with(entry, values, changed, host_twin=False):
    """one of the two entries (or its _host twin: no memspace) with `values` (name -> argument) and some of them changed -> (status, message)"""
    L = _lib().lib()
    names = MEASURE_ARGS if entry == "measure" else SELECT_ARGS
    fn = getattr(L, ("mrcnn_rle_components" if entry == "measure" else "mrcnn_rle_components_select") + ("_host" if host_twin else ""))
    args = {**values, **changed}
    st = fn(*[args[k] for k in names if not (host_twin and k == "memspace")])
    return st, L.mrcnn_last_error().decode()
