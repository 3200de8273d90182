"""The cases of the set-algebra tests (tests/test_rle_combine_host.py, tests/test_gpu_rle_combine.py) and the rule of
include/maskrcnn_hip.h restated in numpy on dense planes: np.logical_or.reduce, np.logical_and.reduce, the parity of the sum, and
first & ~or(rest).

Planes: 1x1, 1x7, 7x1; sides from {31, 32, 33, 63, 64, 65} in both orientations — the word rows of the packed bit box and the encoder's
63-position chunks — one 130x40 plane and one of 1100x9, which is taller than the 1024 rows the kernel folds per pass.  Per plane a
pool of 12 RLEs: empty, full, the four corner pixels, one corner pixel, a checkerboard, a comb (full-height columns under a full top
row: its runs wrap column ends), an ellipse, one that overlaps it, one that does not, and three random planes at density 0.5; every
fourth RLE of the set is re-encoded with zero-length runs.  Groups of 1, 2, 3 and 17 members on every plane and one of 100 members on
the 33x65 plane (drawn from the pool, so duplicates occur), an RLE listed twice, a group whose members are all empty, groups with a
full first member; RLEs shared by many groups; the groups shuffled, so their order is unrelated to the set's.  Deterministic."""
import importlib

import numpy as np

from morph_cases import decode, ellipse, encode, with_zero_runs  # noqa: F401  (decode is the tests')

OR, AND, XOR, DIFF = 0, 1, 2, 3
OPS = {"or": OR, "and": AND, "xor": XOR, "diff": DIFF}
SHAPE, INVALID = 4, 1                        # MRCNN_ERR_SHAPE, MRCNN_ERR_INVALID
SIDES = [31, 32, 33, 63, 64, 65]
SIZES = [(1, 1), (1, 7), (7, 1)] + list(zip(SIDES, SIDES[3:] + SIDES[:3])) + [(130, 40), (1100, 9)]
POOL = ["empty", "full", "corners", "corner_tl", "checkerboard", "comb", "ellipse_a", "ellipse_b", "ellipse_c", "rand0", "rand1", "rand2"]


# ---- the rule on dense planes ------------------------------------------------------------------------------------------------------------
def reference(planes, op):
    """the members' planes, in their order, combined -> a uint8 plane"""
    P = np.stack([np.asarray(p, bool) for p in planes])
    if op == OR:
        R = np.logical_or.reduce(P)
    elif op == AND:
        R = np.logical_and.reduce(P)
    elif op == XOR:
        R = (P.sum(0) & 1).astype(bool)
    else:
        R = P[0] & ~np.logical_or.reduce(P[1:]) if len(P) > 1 else P[0]
    return R.astype(np.uint8)


# ---- contents ----------------------------------------------------------------------------------------------------------------------------
def pool(h, w, rng):
    """the 12 planes of one size, in POOL's order"""
    z = lambda: np.zeros((h, w), np.uint8)
    corners = z(); corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 1
    tl = z(); tl[0, 0] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    comb = z(); comb[:, ::2] = 1; comb[0, :] = 1
    out = [z(), np.ones((h, w), np.uint8), corners, tl, ((yy + xx) & 1).astype(np.uint8), comb,
           ellipse(h, w, h * 0.4, w * 0.4, h * 0.3, w * 0.3), ellipse(h, w, h * 0.55, w * 0.55, h * 0.3, w * 0.3),     # a and b overlap
           ellipse(h, w, h * 0.9, w * 0.9, h * 0.08, w * 0.08)]                                                        # c lies apart from a
    out += [(rng.random((h, w)) < 0.5).astype(np.uint8) for _ in range(3)]
    return out


def groups_of(h, w, rng):
    """[(name, indices into the pool)] for one size"""
    i = POOL.index
    out = [(name, [k]) for k, name in enumerate(POOL)]
    for a, b in (("ellipse_a", "ellipse_b"), ("ellipse_a", "ellipse_c"), ("rand0", "rand1"), ("full", "rand0"), ("rand0", "full"), ("empty", "rand0"),
                 ("rand0", "empty"), ("comb", "checkerboard"), ("checkerboard", "comb"), ("corners", "comb"), ("rand0", "rand0"), ("comb", "comb")):
        out.append((f"{a}+{b}", [i(a), i(b)]))
    out.append(("all_empty", [i("empty")] * 3))
    for names in (("rand0", "rand1", "rand2"), ("ellipse_a", "ellipse_b", "ellipse_c"), ("full", "ellipse_a", "corners")):
        out.append(("+".join(names), [i(n) for n in names]))
    out.append(("g17", rng.integers(0, len(POOL), 17).tolist()))
    if (h, w) == (33, 65):
        out.append(("g100", rng.integers(0, len(POOL), 100).tolist()))
    return out


def all_cases():
    """The whole set for one ragged call: {"runs": [counts per RLE], "planes": [dense plane per RLE], "hs", "ws",
    "groups": [index lists into the set], "names": ["<group>/<h>x<w>" per group]}"""
    rng = np.random.default_rng(23)
    runs, planes, groups, names = [], [], [], []
    for h, w in SIZES:
        base = len(runs)
        for p in pool(h, w, rng):
            c = encode(p)
            runs.append(with_zero_runs(c, rng) if len(runs) % 4 == 1 else c)
            planes.append(p)
        for name, idx in groups_of(h, w, rng):
            groups.append([base + k for k in idx])
            names.append(f"{name}/{h}x{w}")
    order = rng.permutation(len(groups))                         # the groups' order has nothing to do with the set's
    return {"runs": runs, "planes": planes, "hs": np.array([p.shape[0] for p in planes], np.int32), "ws": np.array([p.shape[1] for p in planes], np.int32),
            "groups": [groups[k] for k in order], "names": [names[k] for k in order]}


def flat_set(runs):
    """(counts, run_offsets) of a list of runs"""
    counts = np.concatenate(runs).astype(np.uint32) if len(runs) else np.zeros(1, np.uint32)
    return counts, np.concatenate(([0], np.cumsum([len(c) for c in runs]))).astype(np.int64)


def flat_groups(groups):
    """(group_offsets, members) of a list of index lists"""
    offs = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int64)
    mem = np.array([k for g in groups for k in g], np.int64)
    return offs, (mem if mem.size else np.zeros(1, np.int64))


def only(cases, name):
    """the one group `name` with its own members as a set of its own: (runs, hs, ws, groups, planes)"""
    g = cases["groups"][cases["names"].index(name)]
    used = sorted(set(g))
    return ([cases["runs"][k] for k in used], cases["hs"][used], cases["ws"][used], [[used.index(k) for k in g]], [cases["planes"][k] for k in used])


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def combine_host(counts, offs, hs, ws, goffs, mem, op, capacity=None, fill=None):
    """mrcnn_rle_combine_host with the size query first -> (status, message, counts, run_offsets, areas, bboxes)"""
    L = _lib().lib()
    n, G = len(offs) - 1, len(goffs) - 1
    counts, offs = np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(offs, np.int64)
    hs, ws = (np.ascontiguousarray(a, np.int32) for a in (hs, ws))
    goffs, mem = (np.ascontiguousarray(a, np.int64) for a in (goffs, mem))
    out_offs, areas, boxes = np.zeros(G + 1, np.int64), np.zeros(max(1, G), np.uint32), np.zeros((max(1, G), 4), np.int32)
    head = (counts.ctypes.data, offs.ctypes.data, n, hs.ctypes.data, ws.ctypes.data, goffs.ctypes.data, mem.ctypes.data, G, op)
    if capacity is None:
        st = L.mrcnn_rle_combine_host(*head, None, 0, out_offs.ctypes.data, None, None)
        if st != SHAPE or out_offs[G] == 0:
            return st, L.mrcnn_last_error().decode(), None, out_offs, areas[:G], boxes[:G]
        capacity = int(out_offs[G])
    out = np.zeros(max(1, capacity), np.uint32) if fill is None else np.full(max(1, capacity), fill, np.uint32)
    st = L.mrcnn_rle_combine_host(*head, out.ctypes.data, capacity, out_offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data)
    return st, L.mrcnn_last_error().decode(), out[:int(out_offs[G])] if st == 0 else out, out_offs, areas[:G], boxes[:G]
