"""The cases of the transform tests (tests/test_rle_transform_host.py, tests/test_gpu_rle_transform.py) and the rule of
include/maskrcnn_hip.h restated in numpy on dense planes: the index vectors u(X) and v(Y) from Python's //, which is floor division,
gathered from the zero-padded plane with np.ix_, and .T applied for MRCNN_XF_TRANSPOSE.

Planes: 1x1, 1x7, 7x1; sides from {31, 32, 33, 63, 64, 65} in both orientations — the word rows of the packed bit box — one 130x40
plane, and 1100x9 and 9x1100, which pass the 1024 rows the kernel fills per pass, and do so again after a transposition.  Masks:
combine_cases.pool — empty, full, corners, one corner, checkerboard, the comb whose runs wrap column ends, ellipses, random planes at
density 0.5 — two of them per record in turn; every fourth RLE is re-encoded with zero-length runs.  Records per plane: the identity,
all eight symmetries, a crop inside, crops that reach outside on each side and on all four at once (negative numerators), a window
wholly outside (an empty work box), translations by +-1, +-31, +-32, +-33 into a frame larger by 40, resizes x2, x3, x3/2, x1/2, x1/3,
x2/3, x7/5 under both rules, an anisotropic one, one with a flip, one with a transposition, the plane to 1x1, the 1x1 plane to 65x33, and
twenty random records with |a|, d in 1..7, b in -200..200, random transposition and output sides 1..70.  Deterministic."""
import importlib

import numpy as np

from combine_cases import POOL, flat_set, pool  # noqa: F401  (flat_set is the tests')
from morph_cases import decode, encode, stats, with_zero_runs  # noqa: F401

TRANSPOSE = 1
SHAPE, INVALID = 4, 1                        # MRCNN_ERR_SHAPE, MRCNN_ERR_INVALID
SIDES = [31, 32, 33, 63, 64, 65]
SIZES = [(1, 1), (1, 7), (7, 1)] + list(zip(SIDES, SIDES[3:] + SIDES[:3])) + [(130, 40), (1100, 9), (9, 1100)]     # (31x63 .. 65x33: both orientations)
FACTORS = [(2, 1), (3, 1), (3, 2), (1, 2), (1, 3), (2, 3), (7, 5)]
SHIFTS = [1, -1, 31, -31, 32, -32, 33, -33]


# ---- the rule on dense planes ------------------------------------------------------------------------------------------------------------
def reference(P, xf, oh, ow):
    """the plane P read through the record -> the (oh, ow) uint8 plane"""
    flags, ax, bx, dx, ay, by, dy, _ = (int(v) for v in xf)
    u = np.array([(ax * X + bx) // dx for X in range(ow)], np.int64)     # Python's //: floor, also for negative numerators
    v = np.array([(ay * Y + by) // dy for Y in range(oh)], np.int64)
    Q = np.asarray(P, np.uint8).T if flags & TRANSPOSE else np.asarray(P, np.uint8)      # Out[Y, X] = Q[v(Y), u(X)]
    qh, qw = Q.shape
    Z = np.pad(Q, 1)                                                     # index 0 of the padded plane: outside, 0
    rows = np.where((v >= 0) & (v < qh), v + 1, 0)
    cols = np.where((u >= 0) & (u < qw), u + 1, 0)
    return Z[np.ix_(rows, cols)].astype(np.uint8)


# ---- records -----------------------------------------------------------------------------------------------------------------------------
def rec(flags, ax, bx, dx, ay, by, dy):
    return np.array([flags, ax, bx, dx, ay, by, dy, 0], np.int64)


def symmetry(h, w, transpose, flip_x, flip_y):
    """one of the eight symmetries of the h x w plane -> (record, (oh, ow)); the flips act on the OUTPUT's X and Y"""
    nx, ny = (h, w) if transpose else (w, h)                             # what X and Y index in the source
    return rec(TRANSPOSE if transpose else 0, -1 if flip_x else 1, nx - 1 if flip_x else 0, 1, -1 if flip_y else 1, ny - 1 if flip_y else 0, 1), (ny, nx)


def crop(x, y, ww, wh):
    return rec(0, 1, x, 1, 1, y, 1), (wh, ww)


def place(x0, y0, fh, fw):
    return rec(0, 1, -x0, 1, 1, -y0, 1), (fh, fw)


def resize(h, w, oh, ow, rule):
    if rule == "center":
        return rec(0, 2 * w, w, 2 * ow, 2 * h, h, 2 * oh), (oh, ow)
    return rec(0, w, 0, ow, h, 0, oh), (oh, ow)


def scaled(n, p, q):
    return max(1, n * p // q)


def records_of(h, w, rng):
    """[(name, record, (oh, ow))] for one plane"""
    out = [("identity", *crop(0, 0, w, h))]
    for t in (0, 1):
        for fx in (0, 1):
            for fy in (0, 1):
                out.append((f"sym_t{t}x{fx}y{fy}", *symmetry(h, w, t, fx, fy)))
    hw, hh = max(1, w // 2), max(1, h // 2)
    out.append(("crop_inside", *crop(w // 4, h // 4, hw, hh)))
    out.append(("crop_left", *crop(-3, h // 4, hw + 3, hh)))
    out.append(("crop_right", *crop(w // 2, h // 4, w - w // 2 + 3, hh)))
    out.append(("crop_top", *crop(w // 4, -3, hw, hh + 3)))
    out.append(("crop_bottom", *crop(w // 4, h // 2, hw, h - h // 2 + 3)))
    out.append(("crop_all_sides", *crop(-3, -3, w + 6, h + 6)))
    out.append(("crop_outside", *crop(w + 2, -1, 5, h + 1)))
    for s in SHIFTS:
        out.append((f"shift_{s}", *place(s, -s if abs(s) == 32 else s, h + 40, w + 40)))
    for p, q in FACTORS:
        for rule in ("center", "floor"):
            out.append((f"resize_{p}/{q}_{rule}", *resize(h, w, scaled(h, p, q), scaled(w, p, q), rule)))
    out.append(("resize_aniso", *resize(h, w, scaled(h, 1, 3), 2 * w, "center")))
    ow = scaled(w, 3, 2)
    out.append(("resize_flip", rec(0, -2 * w, w * (2 * ow - 1), 2 * ow, 2 * h, h, 2 * scaled(h, 3, 2)), (scaled(h, 3, 2), ow)))
    tw, th = scaled(h, 3, 2), scaled(w, 2, 3)                            # transposed: X reads the source's rows, Y its columns
    out.append(("resize_transpose", rec(TRANSPOSE, 2 * h, h, 2 * tw, 2 * w, w, 2 * th), (th, tw)))
    out.append(("to_1x1", *resize(h, w, 1, 1, "center")))
    if (h, w) == (1, 1):
        out.append(("1x1_to_65x33", *resize(1, 1, 65, 33, "center")))
    for k in range(20):
        a = rng.integers(1, 8, 2) * rng.choice([-1, 1], 2)
        d = rng.integers(1, 8, 2)
        b = rng.integers(-200, 201, 2)
        out.append((f"random{k}", rec(int(rng.integers(0, 2)), a[0], b[0], d[0], a[1], b[1], d[1]), tuple(int(s) for s in rng.integers(1, 71, 2))))
    return out


def all_cases():
    """The whole set for one ragged call: {"names": ["<record>/<mask>/<h>x<w>"], "runs", "planes" (the sources), "hs", "ws", "ohs", "ows",
    "xf" (n, 8)}"""
    rng = np.random.default_rng(29)
    names, runs, planes, xf, osz = [], [], [], [], []
    turn = 0
    for h, w in SIZES:
        masks = pool(h, w, rng)
        codes = [encode(p) for p in masks]
        for rname, r, (oh, ow) in records_of(h, w, rng):
            for _ in range(2):                                           # two masks of the pool per record, in turn
                m = turn % len(POOL)
                turn += 5                                                # (5 and 12 are coprime: every record meets changing masks)
                runs.append(with_zero_runs(codes[m], rng) if len(runs) % 4 == 1 else codes[m])
                planes.append(masks[m])
                names.append(f"{rname}/{POOL[m]}/{h}x{w}")
                xf.append(r)
                osz.append((oh, ow))
    col = lambda a: np.array(a, np.int32)
    return {"names": names, "runs": runs, "planes": planes, "hs": col([p.shape[0] for p in planes]), "ws": col([p.shape[1] for p in planes]),
            "ohs": col([s[0] for s in osz]), "ows": col([s[1] for s in osz]), "xf": np.stack(xf).astype(np.int64)}


def subset(cases, idx):
    """the cases `idx` as a set of their own: (runs, hs, ws, ohs, ows, xf, planes)"""
    idx = list(idx)
    return ([cases["runs"][k] for k in idx], cases["hs"][idx], cases["ws"][idx], cases["ohs"][idx], cases["ows"][idx], cases["xf"][idx],
            [cases["planes"][k] for k in idx])


def expected(planes, xf, ohs, ows):
    """(counts, run_offsets, areas, bboxes) of the numpy rule for a set"""
    want = [reference(p, r, int(oh), int(ow)) for p, r, oh, ow in zip(planes, xf, ohs, ows)]
    codes = [encode(p) for p in want]
    st = [stats(p) for p in want]
    counts, offs = flat_set(codes)
    return counts[:int(offs[-1])], offs, np.array([s[0] for s in st], np.uint32), np.array([s[1] for s in st], np.int32).reshape(-1, 4), want


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def transform_host(counts, offs, hs, ws, ohs, ows, xf, capacity=None, fill=None):
    """mrcnn_rle_transform_host with the size query first -> (status, message, counts, run_offsets, areas, bboxes)"""
    L = _lib().lib()
    n = len(offs) - 1
    counts, offs = np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(offs, np.int64)
    hs, ws, ohs, ows = (np.ascontiguousarray(a, np.int32) for a in (hs, ws, ohs, ows))
    xf = np.ascontiguousarray(xf, np.int64)
    out_offs, areas, boxes = np.zeros(n + 1, np.int64), np.zeros(max(1, n), np.uint32), np.zeros((max(1, n), 4), np.int32)
    head = (counts.ctypes.data, offs.ctypes.data, n, hs.ctypes.data, ws.ctypes.data, ohs.ctypes.data, ows.ctypes.data, xf.ctypes.data)
    if capacity is None:
        st = L.mrcnn_rle_transform_host(*head, None, 0, out_offs.ctypes.data, None, None)
        if st != SHAPE or out_offs[n] == 0:
            return st, L.mrcnn_last_error().decode(), None, out_offs, areas[:n], boxes[:n]
        capacity = int(out_offs[n])
    out = np.zeros(max(1, capacity), np.uint32) if fill is None else np.full(max(1, capacity), fill, np.uint32)
    st = L.mrcnn_rle_transform_host(*head, out.ctypes.data, capacity, out_offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data)
    return st, L.mrcnn_last_error().decode(), out[:int(out_offs[n])] if st == 0 else out, out_offs, areas[:n], boxes[:n]
